"""svl_lora_merge_f32 / svl_lora_wgrad_f32 on the GPU against their float64 restatement (tests/lora_ref.py).  Outputs are
written between sentinel guard bands, every case runs twice and must agree bit for bit, and no tolerance is picked: the bound
is, per element, gamma(n) times the sum of absolute terms, with n the number of fp32 roundings on the kernel's longest chain
(csrc/lora.hip; every multiply-add there is an explicit fmaf):

  merge  r fused multiply-adds onto 0, then fma(s, acc, W): r + 1 roundings                              n = r + 2 (as stated)
  dB     one chain over e in ascending order, E fused multiply-adds (the zero padding of the last 128-column tile adds exact
         zeros), times s, plus the previous value when accumulating: E + 2 roundings                     n = E + 2
  dA     per 16-row tile one chain of 16 fused multiply-adds and the product with s (17 roundings); the tiles are then added
         in double in tile order (onto the previous value when accumulating) and rounded once: 18 roundings, whatever `rows`
         is.  The double sum's own error, (tiles + 1) * 2^-53 relative, is added to the bound, as is the float64
         reference's (rows * 2^-53).                                                                     n = 16 + 2

With -s each case prints its worst error / bound ratio."""
import ctypes as C

import numpy as np
import pytest
import torch

import lora_ref as R
from small_kernel_ref import GUARD, SENTINEL, guard_intact, guarded

pytestmark = pytest.mark.gpu

AG = 64      # guard elements around the E-wide outputs: the kernels take 16-byte aligned matrices
SHAPES = [(64, 64, 4, "o"), (192, 64, 3, "qv"), (768, 768, 4, "o"), (2304, 768, 16, "o"), (40, 40, 1, "o"), (128, 128, 64, "o")]
IDS = ["64x64r4", "192x64r3-qv", "768x768r4", "2304x768r16", "40x40r1", "128x128r64"]
TILE_ROWS = 16


def _inputs(rows, E, r, targets, seed):
    """W / dW [rows, E] and per row block (one block, or the q | k | v blocks of an in_proj with targets 'qv') A, B"""
    g = torch.Generator().manual_seed(seed)
    nblk = 3 if targets == "qv" else 1
    W = torch.randn(rows, E, generator=g)
    pairs = [(torch.randn(r, E, generator=g), torch.randn(rows // nblk, r, generator=g))
             if (nblk == 1 or "qkv"[i] in targets) else None for i in range(nblk)]
    return W, pairs


def _ratio(got, ref, bound):
    err = np.abs(got.double().cpu().numpy() - ref)
    assert np.isfinite(err).all()
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("s", [1.0, 2.5])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_merge_matches_fp64_within_the_rounding_bound(dev, shape, s):
    from semivl_amd import ops
    rows, E, r, targets = shape
    W, pairs = _inputs(rows, E, r, targets, seed=rows + r)
    ref, mag = R.merge_ref(W.numpy(), [None if p is None else (p[0].numpy(), p[1].numpy()) for p in pairs], s)
    Wd = W.to(dev)
    pd = [None if p is None else (p[0].to(dev), p[1].to(dev)) for p in pairs]
    bufs = []
    for _ in range(2):
        buf, pay = guarded(rows * E, device=dev, guard=AG)
        ops.lora_merge(Wd, pd, s, out=pay.view(rows, E))
        bufs.append(buf)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1]) and guard_intact(bufs[0], rows * E, guard=AG)
    got = bufs[0][AG:AG + rows * E].view(rows, E)
    ratio = _ratio(got, ref, R.gamma(r + 2) * mag)
    print(f"lora_merge rows={rows} E={E} r={r} s={s}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    nblk = len(pairs)
    for i, p in enumerate(pairs):     # a block without a target is a plain copy
        if p is None:
            sl = slice(i * rows // nblk, (i + 1) * rows // nblk)
            assert torch.equal(got[sl], Wd[sl])


@pytest.mark.parametrize("acc", [(False, False), (True, True), (True, False)], ids=["write", "acc", "accB"])
@pytest.mark.parametrize("s", [1.0, 2.5])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_wgrad_matches_fp64_within_the_rounding_bound(dev, shape, s, acc):
    from semivl_amd import ops
    rows_all, E, r, targets = shape
    dW, pairs = _inputs(rows_all, E, r, targets, seed=7 * rows_all + r)
    nblk = len(pairs)
    rows = rows_all // nblk
    dWd = dW.to(dev)
    g = torch.Generator().manual_seed(5)
    worst = [0.0, 0.0]
    for i, p in enumerate(pairs):
        if p is None:
            continue
        A, B = p
        dB0, dA0 = torch.randn(rows, r, generator=g), torch.randn(r, E, generator=g)
        blk = dW[i * rows:(i + 1) * rows]
        dB, dA, magB, magA = R.wgrad_ref(blk.numpy(), A.numpy(), B.numpy(), s, dB0.numpy() if acc[0] else None,
                                         dA0.numpy() if acc[1] else None)
        Ad, Bd = A.to(dev), B.to(dev)
        bufs = []
        for _ in range(2):
            bb, pb = guarded(rows * r, device=dev)
            ba, pa = guarded(r * E, device=dev, guard=AG)
            if acc[0]:
                pb.copy_(dB0.view(-1))
            if acc[1]:
                pa.copy_(dA0.view(-1))
            ops.lora_wgrad(dWd[i * rows:(i + 1) * rows], Ad, Bd, s, out_b=pb.view(rows, r), out_a=pa.view(r, E),
                           accumulate_b=acc[0], accumulate_a=acc[1])
            bufs.append((bb, ba))
        torch.cuda.synchronize()
        assert torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1])
        assert guard_intact(bufs[0][0], rows * r) and guard_intact(bufs[0][1], r * E, guard=AG)
        gb = bufs[0][0][GUARD:GUARD + rows * r].view(rows, r)
        ga = bufs[0][1][AG:AG + r * E].view(r, E)
        tiles = -(-rows // TILE_ROWS)
        worst[0] = max(worst[0], _ratio(gb, dB, R.gamma(E + 2) * magB))
        worst[1] = max(worst[1], _ratio(ga, dA, (R.gamma(TILE_ROWS + 2) + (tiles + 1 + rows) * 2.0 ** -53) * magA))
    print(f"lora_wgrad rows={rows} E={E} r={r} s={s} accumulate={acc}: worst error / bound dB {worst[0]:.3f}, dA {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


@pytest.mark.parametrize("rows,E,r", [(64, 64, 0), (64, 64, 65), (50, 50, 4)], ids=["r0", "r65", "E50"])
def test_unsupported_shapes_are_refused_and_write_nothing(dev, rows, E, r):
    import semivl_amd.lib as L
    lib = L.load()
    rr = max(r, 1)
    W = torch.randn(rows, E, device=dev)
    A, B = torch.randn(rr, E, device=dev), torch.randn(rows, rr, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bo, po = guarded(rows * E, device=dev, guard=AG)
    Ap, Bp = (C.c_void_p * 1)(A.data_ptr()), (C.c_void_p * 1)(B.data_ptr())
    rc = lib.svl_lora_merge_f32(p(W), E, p(po), E, 1, rows, E, r, 1.0, Ap, Bp, rr, st)
    assert rc < 0 and "svl_lora_merge_f32" in L.last_error()
    assert lib.svl_lora_wgrad_ws_floats(rows, E, r) < 0
    bb, pb = guarded(rows * rr, device=dev)
    ba, pa = guarded(rr * E, device=dev, guard=AG)
    ws = torch.full((rows * rr * E,), SENTINEL, device=dev)
    rc = lib.svl_lora_wgrad_f32(p(W), E, p(A), p(B), rr, rows, E, r, 1.0, p(pb), 0, p(pa), 0, p(ws), st)
    assert rc < 0 and "svl_lora_wgrad_f32" in L.last_error()
    torch.cuda.synchronize()
    for buf in (bo, bb, ba, ws):
        assert torch.equal(buf, torch.full_like(buf, SENTINEL))
    assert lib.svl_lora_merge_f32(None, E, p(po), E, 1, rows, E, 4, 1.0, Ap, Bp, rr, st) < 0      # a null pointer
    assert lib.svl_lora_wgrad_f32(p(W), E, None, p(B), rr, rows, E, 4, 1.0, p(pb), 0, p(pa), 0, p(ws), st) < 0
