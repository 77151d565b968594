"""CPU: the float64 restatements of tests/pool_tokens_ref.py against the tensor expressions the kernels stand for in the
DeepLabV3+ head -- `x.view(b, HW, C).mean(1)`, its autograd, `expand` and `sum` -- and a plain fp32 evaluation of the same
expressions inside the derived bounds on the very inputs tests/test_pool_tokens_gpu.py uses."""
import pytest
import torch

import pool_tokens_ref as P


@pytest.mark.parametrize("case", P.CASES + [P.BIG_SUM], ids=str)
def test_gap_restatements(case):
    imgs, HW, C = case
    x, dpool, base = P.inputs(case)
    xd = x.double().requires_grad_(True)
    pool = xd.view(imgs, HW, C).mean(1)
    want, bound = P.gap_fwd_ref(x, imgs, HW)
    assert torch.allclose(want, pool.detach(), rtol=1e-13, atol=1e-15)
    pool.backward(dpool.double())
    wb, bb = P.gap_bwd_ref(dpool, imgs, HW)
    assert torch.allclose(wb, xd.grad, rtol=1e-13, atol=0)
    wa, ba = P.gap_bwd_ref(dpool, imgs, HW, base=base)
    assert torch.allclose(wa, base.double() + xd.grad, rtol=1e-13, atol=1e-15)
    # a plain fp32 evaluation whose only rounding is the last one stays inside the bounds
    assert bool(((pool.detach().float().double() - want).abs() <= bound).all())
    assert bool((((dpool / HW).repeat_interleave(HW, 0).double() - wb).abs() <= bb).all())
    assert bool((((dpool / HW).repeat_interleave(HW, 0) + base).double().sub(wa).abs() <= ba).all())
    assert bool((bound >= 0).all()) and (HW > 1 or torch.equal(want, x.double()))


@pytest.mark.parametrize("case", P.CASES, ids=str)
def test_bcast_restatements(case):
    imgs, HW, C = case
    x, dpool, _ = P.inputs(case)
    v = dpool.clone().requires_grad_(True)
    y = v[:, None, :].expand(imgs, HW, C).reshape(imgs * HW, C)
    assert torch.equal(P.bcast_fwd_ref(dpool, imgs, HW), y.detach())
    want, bound = P.bcast_bwd_ref(x, imgs, HW)
    assert torch.allclose(want, x.double().view(imgs, HW, C).sum(1), rtol=1e-13, atol=1e-15)
    y.backward(x)                                    # autograd of expand: the per-image sum, here in fp32
    assert bool(((v.grad.double() - want).abs() <= P.gamma(max(HW - 1, 1)) / P.gamma(1) * bound).all())


def test_cases_reach_every_path():
    """The case list holds what the kernels branch on: C % 4 != 0, C a multiple of the 64-channel group and a ragged last
    group, HW below / above the row lanes of a block, and launches beyond one pass of the capped grids."""
    Cs, HWs = {c[2] for c in P.CASES}, {c[1] for c in P.CASES}
    assert any(c % 4 for c in Cs) and any(c % P.GAP_CH == 0 for c in Cs) and any(c > P.GAP_CH and c % P.GAP_CH for c in Cs)
    assert min(HWs) == 1 and max(HWs) > 16 * 16
    imgs, HW, C = P.BIG_ELTWISE
    assert C % 4 == 0 and imgs * HW * (C // 4) > P.GRID_CAP * 256
    imgs, HW, C = P.BIG_SUM
    assert imgs * ((C + P.GAP_CH - 1) // P.GAP_CH) > P.GRID_CAP
    assert {off % 4 for _, _, off in P.LAYOUTS} == {0, 3}
