"""CPU proof of tests/sgd_ref.py (the float64 restatement of svl_sgd_step and its fp32 bound) against torch.optim.SGD, and
of the device-free parts of FusedSGD: the reference's two param groups and their state-dict numbering (semivl.py:118-121),
its schedule (semivl.py:330-337) and the optimizer dispatch (semivl.py:118-125)."""
import numpy as np
import pytest
import torch

import sgd_ref as R


def _run_torch_and_ref(case, mode, dtype, steps=3):
    """Steps torch.optim.SGD in `dtype`; before each step restates it from torch's own state.  Yields (step, ref, p, m)."""
    opt, prm = R.torch_sgd(case, mode, dtype)
    gs = R.f32(mode["gscale"])
    for step in range(1, steps + 1):
        p0 = R.flat(case, prm)
        m0 = R.flat(case, [opt.state[q]["momentum_buffer"] for q in prm]) if step > 1 and mode["momentum"] else \
            torch.zeros(case["total"], dtype=torch.float64)
        g = case["gs"][step - 1]
        ref = R.sgd_ref(p0, g, m0 if mode["momentum"] else None, case["seg_off"], case["seg_lr"], case["seg_wd"], case["nseg"],
                        case["total"], mode["momentum"], mode["dampening"], mode["nesterov"], step, gs)
        for q, a, s in zip(prm, case["offs"], case["sizes"]):
            q.grad = (g[a:a + s].to(dtype) * torch.tensor(gs, dtype=dtype)).clone()     # fp32: ONE rounding, the kernel's t1
        opt.step()
        m1 = R.flat(case, [opt.state[q]["momentum_buffer"] for q in prm]).numpy() if mode["momentum"] else None
        yield step, ref, R.flat(case, prm).numpy(), m1


@pytest.mark.parametrize("mode", sorted(R.MODES))
def test_restatement_equals_torch_sgd_in_float64(mode):
    case = R.arena(R.SIZES["ragged"], seed=3)
    for step, ref, p, m in _run_torch_and_ref(case, R.MODES[mode], torch.float64):
        scale = np.abs(ref["p"]).max()
        assert np.abs(ref["p"] - p).max() <= 1e-14 * scale, (mode, step)
        if m is not None:
            assert np.abs(ref["m"] - m).max() <= 1e-14 * np.abs(ref["m"]).max(), (mode, step)
        assert not ref["p"][case["pad"].numpy()].any()


def test_first_step_rule_shows_with_dampening():
    """m = d on step 1 (torch clones the gradient), not (1 - dampening) * d: the two differ by 30 % here."""
    case = R.arena([8], seed=1)
    a = R.sgd_ref(case["p"], case["gs"][0], torch.zeros(8), case["seg_off"], case["seg_lr"], case["seg_wd"], 1, 8, R.MOM, R.DAMP,
                  False, 1)
    b = R.sgd_ref(case["p"], case["gs"][0], torch.zeros(8), case["seg_off"], case["seg_lr"], case["seg_wd"], 1, 8, R.MOM, R.DAMP,
                  False, 2)
    assert np.allclose(b["m"], (1 - R.DAMP) * a["m"], rtol=1e-12) and not np.allclose(a["m"], b["m"], rtol=0.1)
    with pytest.raises(ValueError):
        R.sgd_ref(case["p"], case["gs"][0], torch.zeros(8), case["seg_off"], case["seg_lr"], case["seg_wd"], 1, 8, R.MOM, R.DAMP,
                  True, 1)
    with pytest.raises(ValueError):
        R.sgd_ref(case["p"], case["gs"][0], None, case["seg_off"], case["seg_lr"], case["seg_wd"], 1, 8, R.MOM, 0.0, False, 1)


@pytest.mark.parametrize("mode", sorted(R.MODES))
def test_bound_holds_for_torch_fp32(mode):
    """torch's own fp32 SGD (the same products and sums, fused or not) lies inside the a-priori bound on every element."""
    worst = 0.0
    for sizes in ("ragged", "many"):
        case = R.arena(R.SIZES[sizes], seed=5)
        for step, ref, p, m in _run_torch_and_ref(case, R.MODES[mode], torch.float32):
            live = ~case["pad"].numpy()
            rp = (np.abs(p - ref["p"])[live] / ref["p_bound"][live]).max()
            worst = max(worst, rp)
            if m is not None:
                nz = live & (ref["m_bound"] > 0)
                worst = max(worst, (np.abs(m - ref["m"])[nz] / ref["m_bound"][nz]).max())
    print(f"sgd_ref bound, torch fp32, {mode}: worst error / bound = {worst:.3f} (k = {ref['k']})")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ grouping, schedule, dispatch
class _Stub(torch.nn.Module):
    """backbone.* (one tensor frozen), decode_head.*, clip_encoder.* -- registered in the product model's order."""

    def __init__(self):
        super().__init__()
        self.decode_head = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))
        self.backbone = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3))
        self.clip_encoder = torch.nn.Linear(4, 3)
        self.backbone[0].bias.requires_grad_(False)


def _reference_sgd(model, lr, lr_multi):
    """semivl.py:119-121, verbatim in spirit."""
    return torch.optim.SGD([{"params": model.backbone.parameters(), "lr": lr},
                            {"params": [prm for name, prm in model.named_parameters() if "backbone" not in name],
                             "lr": lr * lr_multi}], lr=lr, momentum=0.9, weight_decay=1e-4)


def test_original_groups_and_indices_equal_torch():
    from semivl_amd.train import sgd_original_groups
    model = _Stub()
    ref = _reference_sgd(model, 0.001, 10.0)
    members, index, groups = sgd_original_groups(model, 0.001, 10.0)
    assert [[id(p) for _, p in mem] for mem in members] == [[id(p) for p in g["params"]] for g in ref.param_groups]
    sd = ref.state_dict()
    assert [[index[n] for n, _ in mem] for mem in members] == [g["params"] for g in sd["param_groups"]]
    assert [n for n, _ in members[0]] == ["backbone." + n for n, _ in model.backbone.named_parameters()]
    assert any(n.startswith("clip_encoder.") for n, _ in members[1]) and "backbone.0.bias" in index
    # the arena: what can receive a gradient, in named_parameters() order, each tensor with its group's lr
    named = dict(model.named_parameters())
    assert [g["name"] for g in groups] == [n for n, p in named.items() if p.requires_grad and not n.startswith("clip_encoder.")]
    assert "backbone.0.bias" not in [g["name"] for g in groups]
    for g in groups:
        k = 0 if g["name"].startswith("backbone.") else 1
        assert g["group"] == k and g["lr"] == ref.param_groups[k]["lr"] and g["weight_decay"] == 1e-4
        assert g["param"] is named[g["name"]]
    # torch's state after a step is keyed by exactly the indices of the arena tensors
    for g in groups:
        g["param"].grad = torch.ones_like(g["param"])
    ref.step()
    assert sorted(ref.state_dict()["state"]) == sorted(index[g["name"]] for g in groups)


def test_original_groups_refuse_a_parameter_in_neither_group():
    from semivl_amd.train import sgd_original_groups
    model = _Stub()
    model.side = torch.nn.Module()
    model.side.backbone_adapter = torch.nn.Linear(2, 2)          # name contains 'backbone', not under model.backbone
    with pytest.raises(ValueError, match="side.backbone_adapter"):
        sgd_original_groups(model, 0.001, 10.0)


@pytest.mark.parametrize("iters", [0, 3, 9, 10, 11, 57, 99])
def test_original_schedule_is_the_reference_arithmetic(iters):
    from semivl_amd.train import sgd_original_lr
    cfg = dict(lr=0.001, lr_multi=10.0, warmup_iters=10, warmup_ratio=1e-6)
    scheduler_max_iters = 100
    # semivl.py:331-337
    if iters < cfg['warmup_iters']:
        k = (1 - iters / cfg['warmup_iters']) * (1 - cfg['warmup_ratio'])
        lr = cfg['lr'] * (1 - k)
    else:
        lr = cfg['lr'] * (1 - iters / scheduler_max_iters) ** 0.9
    assert sgd_original_lr(cfg["lr"], cfg["lr_multi"], iters, scheduler_max_iters, 10, 1e-6) == (lr, lr * cfg['lr_multi'])


def test_dispatch(monkeypatch):
    from semivl_amd import optim as T
    with pytest.raises(ValueError, match="Adagrad"):
        T.build_optimizer(_Stub(), dict(type="Adagrad", lr=0.1))
    with pytest.raises(AssertionError):
        T.FusedAdamW(_Stub(), dict(type="SGD", lr=0.1))          # called directly it keeps its assertion
    with pytest.raises(ValueError, match="[Nn]esterov"):
        T.build_optimizer(_Stub(), dict(type="SGD", lr=0.1, momentum=0.9, dampening=0.1, nesterov=True))
    seen = []

    class Adam:
        def __init__(self, model, ocfg, ema_decay=None):
            seen.append(("AdamW", ocfg, ema_decay))

    class Sgd:
        def __init__(self, model, ocfg, ema_decay=None):
            seen.append(("SGD", ocfg, ema_decay))

        @classmethod
        def original(cls, model, lr, lr_multi, momentum=0.9, weight_decay=1e-4, ema_decay=None):
            seen.append(("original", lr, lr_multi, momentum, weight_decay, ema_decay))

    monkeypatch.setattr(T, "FusedAdamW", Adam)
    monkeypatch.setattr(T, "FusedSGD", Sgd)
    m = _Stub()
    T.optimizer_from_cfg(m, dict(lr=0.001, lr_multi=10.0))
    T.optimizer_from_cfg(m, dict(lr=0.001, lr_multi=10.0, optimizer=dict(type="SGD", lr=0.1)), ema_decay=0.99)
    T.optimizer_from_cfg(m, dict(optimizer=dict(type="AdamW", lr=0.1)))
    T.optimizer_from_cfg(m, dict(optimizer=dict(lr=0.2)))
    T.build_optimizer(m, dict(type="SGD", lr=0.3))
    assert seen == [("original", 0.001, 10.0, 0.9, 1e-4, None), ("SGD", dict(type="SGD", lr=0.1), 0.99),
                    ("AdamW", dict(type="AdamW", lr=0.1), None), ("AdamW", dict(lr=0.2), None),
                    ("SGD", dict(type="SGD", lr=0.3), None)]
