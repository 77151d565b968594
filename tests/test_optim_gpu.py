"""The arena both fused optimizers build (semivl_amd/optim.py::ArenaOptimizer) on the tiny fixture model, and the ordering of
a load_state_dict() behind a queued poly_lr() copy."""
import pytest
import torch

from golden_util import build_hip, fixture_state, load_fixture

pytestmark = pytest.mark.gpu


def _tiny(dev):
    z, c = load_fixture("tiny")
    hip = build_hip(c)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    return hip.to(dev)


def test_adamw_and_sgd_build_the_same_arena(dev):
    from semivl_amd.optim import FusedAdamW, FusedSGD
    from semivl_amd.synthetic import exp40_cfg
    ocfg = exp40_cfg()["optimizer"]
    common = dict(lr=ocfg["lr"], weight_decay=ocfg["weight_decay"], paramwise_cfg=dict(custom_keys=ocfg["paramwise_cfg"]["custom_keys"]))
    a = FusedAdamW(_tiny(dev), dict(type="AdamW", **common))
    s = FusedSGD(_tiny(dev), dict(type="SGD", momentum=0.9, **common))
    assert a.total == s.total and a.all_params == s.all_params
    assert [g["name"] for g in a.groups] == [g["name"] for g in s.groups] and a.param_groups is a.groups
    for name in ("seg_off", "seg_wd", "seg_lr", "p"):
        assert torch.equal(getattr(a, name), getattr(s, name)), name
    assert a.seg_off.dtype == torch.int64 and a.seg_lr.dtype == a.seg_wd.dtype == a.p.dtype == torch.float32
    assert len(set(a.seg_lr.tolist())) >= 2                         # the custom keys bite
    sizes = [g["param"].numel() for g in a.groups]
    assert any(n % 4 for n in sizes), "the fixture must exercise the padding"
    off = a.seg_off.tolist()
    assert off[-1] == a.total and all(o % 4 == 0 for o in off)
    for opt in (a, s):
        live = torch.zeros(opt.total, dtype=torch.bool, device=dev)
        for g, o, n in zip(opt.groups, off, sizes):
            prm = g["param"]
            assert prm.data.data_ptr() == opt.p.data_ptr() + 4 * o and prm.main_grad.data_ptr() == opt.g.data_ptr() + 4 * o, g["name"]
            assert prm.main_grad.shape == prm.shape and prm.data.is_contiguous() and g["initial_lr"] == g["lr"]
            live[o:o + n] = True
        assert not live.all() and not opt.p[~live].any() and opt.p[live].any()
        assert not opt.g.any() and not opt.m.any() and opt.ema is None and opt.step_count == 0
    assert not a.v.any() and not hasattr(s, "v") and not hasattr(a, "momentum")


def test_load_state_dict_is_ordered_behind_a_queued_poly_lr(dev):
    from semivl_amd.optim import FusedAdamW
    from semivl_amd.synthetic import exp40_cfg
    ocfg = exp40_cfg()["optimizer"]
    opt, other = FusedAdamW(_tiny(dev), ocfg), FusedAdamW(_tiny(dev), ocfg)
    other.poly_lr(30, 100)
    sd = other.state_dict()
    opt.poly_lr(5, 100, warmup_iters=10)                 # its copy from the pinned buffer is queued ...
    opt.load_state_dict(sd)                              # ... when the load rewrites that buffer
    torch.cuda.synchronize()
    loaded = [sd["param_groups"][j]["lr"] for j, (_, ai) in enumerate(other.all_params) if ai is not None]
    assert loaded == [g["lr"] for g in other.groups] == [g["lr"] for g in opt.groups]
    assert torch.equal(opt.seg_lr.cpu(), torch.tensor(loaded, dtype=torch.float32))
    assert torch.equal(opt.seg_lr, other.seg_lr)
    outside = next(sd["param_groups"][j] for j, (_, ai) in enumerate(other.all_params) if ai is None)
    assert opt._lr_factor == outside["lr"] / outside["initial_lr"] and abs(opt._lr_factor - other._lr_factor) < 1e-12
    assert opt._lr_factor != 1.0 and opt.step_count == 0


def test_adamw_loads_the_compact_layout(dev):
    """One group per ARENA tensor (this package's early checkpoints) next to the one-per-model-tensor layout."""
    from semivl_amd.optim import FusedAdamW
    from semivl_amd.synthetic import exp40_cfg
    ocfg = exp40_cfg()["optimizer"]
    a, b = FusedAdamW(_tiny(dev), ocfg), FusedAdamW(_tiny(dev), ocfg)
    torch.manual_seed(0)
    for g in a.groups:                                   # through the views: the padding lanes stay zero
        g["param"].main_grad.copy_(torch.randn(g["param"].shape) * 0.1)
    a.step()
    a.poly_lr(3, 10)
    sd = a.state_dict()
    keep = [j for j, (_, ai) in enumerate(a.all_params) if ai is not None]
    assert 0 < len(keep) < len(a.all_params) and sorted(sd["state"]) == keep
    compact = dict(state={i: sd["state"][j] for i, j in enumerate(keep)},
                   param_groups=[dict(sd["param_groups"][j], params=[i]) for i, j in enumerate(keep)])
    b.load_state_dict(compact)
    assert b.step_count == 1 and b._lr_factor == 1.0    # no group outside the arena to recover the factor from
    assert torch.equal(b.m, a.m) and torch.equal(b.v, a.v) and torch.equal(b.seg_lr, a.seg_lr) and a.m.any() and a.v.any()
    assert [g["lr"] for g in b.groups] == [g["lr"] for g in a.groups]
    with pytest.raises(AssertionError, match="does not match this model"):
        b.load_state_dict(dict(state={}, param_groups=sd["param_groups"][:3]))
