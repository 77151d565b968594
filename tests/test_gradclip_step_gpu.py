"""Gradient-norm clipping through the optimizers and the two training steps on the tiny VLG model (the fixture of
tests/test_sgd_gpu.py), exact fp32 GEMMs (mode 0) and the split emulation (mode 6).  Every run starts from the same state and
the step is reproducible bit for bit, so the clipped run can be held to an unclipped run that is GIVEN the scale the clip
formed: parameters, optimizer state and EMA bit-equal.  grad_stats itself is held to the float64 restatement
(tests/gradclip_ref.py) with the kernel tests' bound."""
import math

import pytest
import torch

import gradclip_ref as R
import sgd_ref as S
from golden_util import build_hip, fixture_batch, fixture_fp_masks, fixture_state, load_fixture

pytestmark = pytest.mark.gpu

CFG = dict(conf_thresh=0.05, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
           maskclip_consistency_lambda=[0.1, 0])
LR, LR_MULTI, WD = 2.0 ** -10, 10.0, S.f32(1e-4)
ADAMW = dict(type="AdamW", lr=1e-3, weight_decay=0.01)
SCENARIOS = {                      # (training step, optimizer)
    "semivl-adamw": ("semivl", "adamw"),
    "supervised-adamw": ("supervised", "adamw"),
    "semivl-sgd": ("semivl", "sgd"),
}


def _tiny(dev):
    z, c = load_fixture("tiny")
    hip = build_hip(c)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    return hip.to(dev), z, c


def _optimizer(kind, hip, grad_clip):
    from semivl_amd.train import FusedAdamW, FusedSGD
    if kind == "adamw":
        return FusedAdamW(hip, ADAMW, ema_decay=0.99, grad_clip=grad_clip)
    return FusedSGD.original(hip, LR, LR_MULTI, weight_decay=WD, ema_decay=0.99, grad_clip=grad_clip)


def _step(dev, step, opt_kind, grad_clip=None, grad_scale=None, reducer=None, opt=None, hip=None):
    """One training step of a fresh tiny model; returns the optimizer (arena, state and grad_stats on it) and aux."""
    from semivl_amd.train import semivl_train_step, supervised_train_step
    z, c = load_fixture("tiny")
    hip = _tiny(dev)[0] if hip is None else hip
    opt = _optimizer(opt_kind, hip, grad_clip) if opt is None else opt
    if grad_scale is not None:
        opt.grad_scale = grad_scale
    red = reducer(opt) if reducer is not None else None
    opt._p0, opt._applied_lr = opt.p.clone(), opt.seg_lr.clone()
    batch = {k: v.to(dev) for k, v in fixture_batch(z, c).items()}
    if step == "semivl":
        _, aux = semivl_train_step(hip, batch, 3, 50, CFG, optimizer=opt, reducer=red, return_aux=True,
                                   fp_masks=[m.to(dev) for m in fixture_fp_masks(z, c)])
    else:
        _, aux = supervised_train_step(hip, dict(img_x=batch["img_x"], mask_x=batch["mask_x"]), 3, 50, CFG, optimizer=opt,
                                       reducer=red, return_aux=True)
    torch.cuda.synchronize()
    return opt, aux


def _state(opt):
    return [t for t in (opt.p, getattr(opt, "m", None), getattr(opt, "v", None), opt.ema) if t is not None]


def _bit_equal(a, b):
    sa, sb = _state(a), _state(b)
    return len(sa) == len(sb) >= 3 and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(sa, sb))


def _stats_ratio(stats, g, max_norm, norm_type, gscale):
    """Worst |grad_stats[k] - restatement| / ((2^-24 + n 2^-52) |restatement|), k = 0..2; the flag exact."""
    ref = R.clip_ref(g, max_norm, norm_type, gscale)
    got = [float(v) for v in stats.double().cpu()]
    assert got[3] == 0.0 and not ref[3]
    return max(abs(got[k] - ref[k]) / R.relative_bound(ref[k], g.numel()) for k in range(3))


@pytest.mark.parametrize("mode", [0, 6])
@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_clipped_step_equals_the_step_given_its_scale(dev, scenario, mode):
    from semivl_amd import ops
    step, kind = SCENARIOS[scenario]
    ops.set_gemm_emulation(mode)
    try:
        # A: no clip.  The arena's gradient stays intact until the next zero_grad: its float64 norm n
        a, aux_a = _step(dev, step, kind)
        assert a.grad_clip is None and a.grad_stats is None and "grad_stats" not in aux_a
        n = R.clip_ref(a.g, math.inf)[0]
        assert math.isfinite(n) and n > 0
        # B: the same step with max_norm = n / 2
        max_norm = R.f32(0.5 * n)
        b, aux_b = _step(dev, step, kind, grad_clip=dict(max_norm=max_norm))
        assert torch.equal(a.g, b.g), "the step is not reproducible: the comparison below would mean nothing"
        assert aux_b["grad_stats"] is b.grad_stats and b.grad_stats.shape == (4,) and b.grad_stats.is_cuda
        assert set(aux_b) - {"grad_stats"} == set(aux_a)
        ratio = _stats_ratio(b.grad_stats, a.g, max_norm, 2.0, 1.0)
        coef = float(b.grad_stats[1])
        print(f"{scenario} mode {mode}: norm {float(b.grad_stats[0]):.6g}, coef {coef:.7f}; grad_stats error / bound = "
              f"{ratio:.3f}")
        assert ratio <= 1.0 and abs(coef - 0.5 * n / (n + 1e-6)) <= 2.0 ** -23
        assert not _bit_equal(a, b), "the clip changed nothing"
        # C: no clip, grad_scale = the fp32 value B applied
        c, _ = _step(dev, step, kind, grad_scale=float(b.grad_stats[2]))
        assert _bit_equal(b, c), "the clipped step differs from the unclipped step given its scale"
        # B': a clip that does not bite is the unclipped step
        b2, _ = _step(dev, step, kind, grad_clip=dict(max_norm=R.f32(2.0 * n)))
        assert float(b2.grad_stats[1]) == 1.0 and float(b2.grad_stats[2]) == 1.0 and _bit_equal(a, b2)
        # max_norm = inf only reports: here the max norm, which is exact
        r, _ = _step(dev, step, kind, grad_clip=dict(max_norm=math.inf, norm_type="inf"))
        assert _bit_equal(a, r) and float(r.grad_stats[0]) == float(a.g.abs().max()) and float(r.grad_stats[1]) == 1.0
        # configuration, not state: the state dict of the clipping optimizer has the keys of the plain one
        assert set(b.state_dict()) == set(a.state_dict())
    finally:
        ops.set_gemm_emulation(0)


def test_set_grad_clip_switches_between_steps(dev):
    """set_grad_clip on a live optimizer: the scratch and grad_stats are allocated once and kept; None switches it off."""
    from semivl_amd.train import FusedAdamW
    hip, z, c = _tiny(dev)
    opt = FusedAdamW(hip, ADAMW)
    assert opt.grad_clip is None and opt.grad_stats is None
    opt.set_grad_clip(3.0)
    stats, ws = opt.grad_stats, opt._clip_ws
    assert opt.grad_clip == dict(max_norm=3.0, norm_type=2.0) and stats is not None and ws.dtype == torch.float64
    opt.set_grad_clip(0.5, norm_type="inf")
    assert opt.grad_clip == dict(max_norm=0.5, norm_type=math.inf) and opt.grad_stats is stats and opt._clip_ws is ws
    opt.g.copy_(R.values("normal", opt.total, 9).to(dev))
    g = opt.g.clone()
    opt.step()
    assert torch.equal(opt.g, g), "the clip must not rewrite the gradient"
    assert _stats_ratio(stats, g, 0.5, "inf", 1.0) <= 1.0 and float(stats[1]) < 1.0
    with pytest.raises(ValueError):
        opt.set_grad_clip(-1.0)
    with pytest.raises(NotImplementedError):
        opt.set_grad_clip(1.0, norm_type=1)
    assert opt.grad_clip == dict(max_norm=0.5, norm_type=math.inf)
    opt.set_grad_clip(None)
    assert opt.grad_clip is None and opt.grad_stats is None


def test_data_parallel_norm_is_that_of_the_averaged_gradient(dev):
    """GradAllReducer's world = 2 / injected-collective hooks ('SUM over two ranks holding the same gradient' = x 2 on the
    communication stream, grad_scale = 1 / 2): the reported norm is HALF the norm of the doubled arena -- the norm of the
    mean -- and the update is the one sgd_ref gives for the scale the clip formed, which (x 2 and x 1/2 being exact) is also
    the single-process clipped step bit for bit."""
    from semivl_amd.train import GradAllReducer

    class Work:
        def __init__(self, ev):
            self.ev = ev

        def wait(self):
            torch.cuda.current_stream().wait_event(self.ev)

    calls = []

    def two_identical_ranks(g):
        calls.append(g.numel())
        g.mul_(2.0)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return Work(ev)

    a, _ = _step(dev, "semivl", "sgd")
    n = R.clip_ref(a.g, math.inf)[0]
    max_norm = R.f32(0.5 * n)
    single, _ = _step(dev, "semivl", "sgd", grad_clip=dict(max_norm=max_norm))
    dp, aux = _step(dev, "semivl", "sgd", grad_clip=dict(max_norm=max_norm),
                    reducer=lambda opt: GradAllReducer(opt, bucket_mb=0.25, world=2, collective=two_identical_ranks))
    assert dp.grad_scale == 0.5 and len(calls) >= 2
    assert torch.equal(dp.g, 2.0 * a.g), "the arena holds the sum over the two ranks"
    doubled = R.clip_ref(dp.g, math.inf)[0]
    ratio = _stats_ratio(dp.grad_stats, dp.g, max_norm, 2.0, 0.5)
    print(f"GradAllReducer world 2: norm {float(dp.grad_stats[0]):.6g} (doubled arena {doubled:.6g}); grad_stats error / "
          f"bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert abs(float(dp.grad_stats[0]) - 0.5 * doubled) <= R.relative_bound(0.5 * doubled, dp.total)
    assert aux["grad_stats"] is dp.grad_stats
    ref = S.sgd_ref(dp._p0, dp.g, torch.zeros(dp.total), dp.seg_off, dp._applied_lr, dp.seg_wd, len(dp.groups), dp.total,
                    dp.momentum, dp.dampening, dp.nesterov, 1, float(dp.grad_stats[2]))
    err = (dp.p.double().cpu().numpy() - ref["p"])
    live = ref["p_bound"] > 0
    worst = float((abs(err[live]) / ref["p_bound"][live]).max())
    print(f"GradAllReducer world 2, clipped SGD step: worst error / bound = {worst:.3f}")
    assert worst <= 1.0 and not abs(err[~live]).any()
    assert torch.equal(dp.grad_stats[:2], single.grad_stats[:2]) and float(dp.grad_stats[2]) == 0.5 * float(single.grad_stats[2])
    assert _bit_equal(dp, single)


@pytest.mark.parametrize("branch", ["optimizer", "original"])
def test_optimizer_from_cfg_switches_the_clip_on(dev, branch):
    """cfg['optimizer_config'] = dict(grad_clip=dict(max_norm=1.0)) through optimizer_from_cfg: the step launches the norm
    pass and grad_stats is the restatement's; the same cfg without the key launches what it launched before -- no
    svl_grad_clip_f32 in the ops-level profile, no grad_stats, aux without the key."""
    from semivl_amd import ops
    from semivl_amd.train import FusedAdamW, FusedSGD, optimizer_from_cfg
    base = dict(optimizer=ADAMW) if branch == "optimizer" else dict(lr=LR, lr_multi=LR_MULTI)
    seen = {}
    # (the tiny model's gradient norm is below 1: `live` is the same cfg with a max_norm that bites)
    for tag, extra in (("on", dict(optimizer_config=dict(grad_clip=dict(max_norm=1.0)))), ("off", {}),
                       ("none", dict(optimizer_config=dict(grad_clip=None))),
                       ("live", dict(optimizer_config=dict(type="OptimizerHook", grad_clip=dict(max_norm=0.01, norm_type=2))))):
        hip, _, _ = _tiny(dev)
        opt = optimizer_from_cfg(hip, dict(base, **extra))
        assert isinstance(opt, FusedAdamW if branch == "optimizer" else FusedSGD)
        ops.PROFILE = {}
        try:
            opt, aux = _step(dev, "semivl", None, opt=opt, hip=hip)
            seen[tag] = (opt, aux, {k: len(v) for k, v in ops.PROFILE.items()})
        finally:
            ops.PROFILE = None
    opt, aux, prof = seen["on"]
    assert opt.grad_clip == dict(max_norm=1.0, norm_type=2.0) and prof.get("grad_clip") == 1
    ratio = _stats_ratio(opt.grad_stats, opt.g, 1.0, 2.0, 1.0)
    print(f"optimizer_from_cfg ({branch}), max_norm 1.0: norm {float(opt.grad_stats[0]):.6g}, coef "
          f"{float(opt.grad_stats[1]):.7f}; grad_stats error / bound = {ratio:.3f}")
    assert ratio <= 1.0 and aux["grad_stats"] is opt.grad_stats
    for tag in ("off", "none"):
        off, aux_off, prof_off = seen[tag]
        assert off.grad_clip is None and off.grad_stats is None and "grad_stats" not in aux_off
        assert "grad_clip" not in prof_off
        assert {k: v for k, v in prof.items() if k != "grad_clip"} == prof_off, "the rest of the step's launches moved"
        assert torch.equal(off.g, opt.g)
    assert _bit_equal_p(seen["off"][0], opt) == (float(opt.grad_stats[1]) == 1.0)
    live = seen["live"][0]
    assert live.grad_clip == dict(max_norm=0.01, norm_type=2.0) and torch.equal(live.g, opt.g)
    assert _stats_ratio(live.grad_stats, live.g, 0.01, 2.0, 1.0) <= 1.0 and float(live.grad_stats[1]) < 1.0
    assert not _bit_equal_p(seen["off"][0], live), "a clip that bites must change the update"


def _bit_equal_p(a, b):
    return torch.equal(a.p.view(torch.int32), b.p.view(torch.int32))
