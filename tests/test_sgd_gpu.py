"""svl_sgd_step on the GPU against tests/sgd_ref.py (float64 restatement + a-priori fp32 bound, proven on the CPU by
tests/test_sgd_ref.py), and FusedSGD through the tiny model's training step against torch.optim.SGD built the reference's way
(semivl.py:118-121).  The worst error / bound ratio of every kernel case is printed (-s)."""
import numpy as np
import pytest
import torch

import sgd_ref as R
from golden_util import build_hip, fixture_batch, fixture_fp_masks, fixture_state, load_fixture

pytestmark = pytest.mark.gpu

ONE_PASS = 2048 * 256 * 4        # floats one trip of svl_sgd_step's capped grid covers (csrc/optim.hip: SGD_GRID_CAP x SGD_TRIP)
BIG = [1500001, 3, 2 * ONE_PASS + 77, 5, 130000]          # > 2 passes; boundaries inside the first, the third and the last trip


def _guarded(src, dev):
    buf = torch.full((src.numel() + 2 * R.AGUARD,), R.SENTINEL, dtype=torch.float32, device=dev)
    buf[R.AGUARD:R.AGUARD + src.numel()] = src.to(dev)
    return buf, buf[R.AGUARD:R.AGUARD + src.numel()]


def _intact(buf, n):
    return bool((buf[:R.AGUARD] == R.SENTINEL).all()) and bool((buf[R.AGUARD + n:] == R.SENTINEL).all())


def _ratio(got, want, bound):
    """Worst |got - want| / bound; an element whose bound is 0 (every term is 0: the padding) must be exact."""
    err = np.abs(got.double().cpu().numpy() - want)
    zero = bound == 0
    assert not err[zero].any(), "an element with no non-zero term moved"
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def _kernel_case(dev, sizes, mode, with_ema, seed):
    from semivl_amd import ops
    case = R.arena(sizes, seed)
    n, md = case["total"], R.MODES[mode]
    gen = torch.Generator().manual_seed(seed + 1)
    pb, p = _guarded(case["p"], dev)
    mb, m = _guarded(torch.zeros(n), dev)
    eb, e = _guarded(torch.randn(n, generator=gen) * ~case["pad"], dev)
    has_m = md["momentum"] != 0
    tabs = [case[k].to(dev) for k in ("seg_off", "seg_lr", "seg_wd")]
    worst = 0.0
    for step in (1, 2, 3):
        g = case["gs"][step - 1].to(dev)
        before = [t.clone() for t in (p, m, e)]
        ref = R.sgd_ref(p, g, m if has_m else None, case["seg_off"], case["seg_lr"], case["seg_wd"], case["nseg"], n,
                        md["momentum"], md["dampening"], md["nesterov"], step, md["gscale"], e if with_ema else None, 0.99)
        outs = []
        for _ in range(2):                                  # twice from the same state: bit for bit
            for t, b in zip((p, m, e), before):
                t.copy_(b)
            ops.sgd_step(p, g, m if has_m else None, *tabs, case["nseg"], md["momentum"], md["dampening"], md["nesterov"], step,
                         md["gscale"], e if with_ema else None, 0.99)
            outs.append([t.clone() for t in (p, m, e)])
        assert all(torch.equal(a, b) for a, b in zip(*outs)), (mode, step)
        worst = max(worst, _ratio(p, ref["p"], ref["p_bound"]))
        if has_m:
            worst = max(worst, _ratio(m, ref["m"], ref["m_bound"]))
        else:
            assert torch.equal(m, before[1])
        if with_ema:
            worst = max(worst, _ratio(e, ref["ema"], ref["ema_bound"]))
        else:
            assert torch.equal(e, before[2])
    pad = case["pad"].to(dev)
    assert not p[pad].any() and not m[pad].any() and not e[pad].any(), "padding lanes must stay exactly 0"
    assert _intact(pb, n) and _intact(mb, n) and _intact(eb, n), "guard bands written"
    return worst


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("mode", sorted(R.MODES))
@pytest.mark.parametrize("sizes", sorted(R.SIZES))
def test_sgd_step_within_bound(dev, sizes, mode, with_ema):
    worst = _kernel_case(dev, R.SIZES[sizes], mode, with_ema, seed=11)
    print(f"svl_sgd_step {sizes}/{mode}/{'ema' if with_ema else 'plain'}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mode,with_ema", [("dampening", True), ("nesterov", False)])
def test_sgd_step_beyond_one_pass_of_the_grid(dev, mode, with_ema):
    assert sum((s + 3) // 4 * 4 for s in BIG) > 2 * ONE_PASS
    worst = _kernel_case(dev, BIG, mode, with_ema, seed=12)
    print(f"svl_sgd_step big/{mode}/{'ema' if with_ema else 'plain'}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_sgd_step_refusals(dev):
    from semivl_amd import lib as L
    from semivl_amd import ops
    case = R.arena([8], 1)
    p, g, m = case["p"].to(dev), case["gs"][0].to(dev), torch.zeros(8, device=dev)
    tabs = [case[k].to(dev) for k in ("seg_off", "seg_lr", "seg_wd")]
    p0 = p.clone()

    def status(m_, momentum, dampening, nesterov):
        return L.load().svl_sgd_step(ops._p(p), ops._p(g), ops._p(m_), *[ops._p(t) for t in tabs], 1, 8, momentum, dampening,
                                     nesterov, 1, 1.0, None, 0.0, ops._st())
    assert status(m, 0.9, 0.3, 1) == -1 and "nesterov" in L.last_error()
    assert status(m, 0.0, 0.0, 1) == -1 and "nesterov" in L.last_error()
    assert status(None, 0.9, 0.0, 0) == -1 and "momentum" in L.last_error()
    with pytest.raises(RuntimeError, match="svl_sgd_step"):
        ops.sgd_step(p, g, None, *tabs, 1, 0.9, 0.0, False, 1)
    assert status(None, 0.0, 0.0, 0) == 0                    # no momentum: no buffer needed
    torch.cuda.synchronize()
    assert not torch.equal(p, p0)


# ------------------------------------------------------------------------------------------------ model level
CFG = dict(conf_thresh=0.05, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
           maskclip_consistency_lambda=[0.1, 0])
# fp32 numbers whose products are fp32 numbers too: the cast at the arena's seg_lr / seg_wd is then exact and a comparison
# with torch in float64 is a comparison of the update alone
LR, LR_MULTI, WD = 2.0 ** -10, 10.0, R.f32(1e-4)


def _tiny(dev=None):
    z, c = load_fixture("tiny")
    hip = build_hip(c)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    return (hip.to(dev) if dev is not None else hip), z, c


def _train_step(hip, z, c, dev, opt, it, total, red=None, cfg=CFG):
    from semivl_amd.train import semivl_train_step
    batch = {k: v.to(dev) for k, v in fixture_batch(z, c).items()}
    return semivl_train_step(hip, batch, it, total, cfg, optimizer=opt, reducer=red,
                             fp_masks=[m.to(dev) for m in fixture_fp_masks(z, c)])


def _reference_sgd(model, lr, lr_multi):
    """semivl.py:119-121 (weight decay 1e-4 as the fp32 number the arena holds)"""
    return torch.optim.SGD([{"params": model.backbone.parameters(), "lr": lr},
                            {"params": [prm for name, prm in model.named_parameters() if "backbone" not in name],
                             "lr": lr * lr_multi}], lr=lr, momentum=0.9, weight_decay=WD)


def _arena_ref(opt, p0, step, gscale=1.0, m0=None):
    return R.sgd_ref(p0, opt.g, m0 if m0 is not None else torch.zeros(opt.total), opt.seg_off, opt._applied_lr, opt.seg_wd,
                     len(opt.groups), opt.total, opt.momentum, opt.dampening, opt.nesterov, step, gscale)


@pytest.fixture(scope="module")
def original_step(dev):
    """ONE training step of the tiny model with FusedSGD.original (iters 3 of 50, warm-up 10)."""
    from semivl_amd.train import FusedSGD
    hip, z, c = _tiny(dev)
    opt = FusedSGD.original(hip, LR, LR_MULTI, weight_decay=WD)
    p0 = opt.p.clone()
    opt._applied_lr = opt.seg_lr.clone()          # the lr this step runs with (poly_lr rewrites seg_lr after it)
    losses = _train_step(hip, z, c, dev, opt, 3, 50, cfg=dict(CFG, warmup_iters=10, warmup_ratio=1e-6))
    torch.cuda.synchronize()
    return dict(opt=opt, p0=p0, losses=losses, hip=hip)


def test_original_step_equals_torch_sgd_built_the_reference_way(dev, original_step):
    """The arena after the step against torch.optim.SGD (float64, so that the bound of the fp32 chain applies to the
    difference as it stands), built as semivl.py:119-121 builds it on a CPU copy of the model and given the arena's gradients."""
    opt, p0 = original_step["opt"], original_step["p0"]
    assert torch.isfinite(original_step["losses"]).all() and opt.g.abs().max() > 0
    cpu, _, _ = _tiny()
    cpu.double()
    ref_opt = _reference_sgd(cpu, LR, LR_MULTI)
    named = dict(cpu.named_parameters())
    for g_ in opt.groups:
        named[g_["name"]].grad = g_["param"].main_grad.detach().double().cpu()
    ref_opt.step()
    ref = _arena_ref(opt, p0, 1)
    off = opt.seg_off.tolist()
    worst = 0.0
    for i, g_ in enumerate(opt.groups):
        sl = slice(off[i], off[i] + g_["param"].numel())
        want = named[g_["name"]].detach().reshape(-1).numpy()
        assert np.abs(ref["p"][sl] - want).max() <= 1e-14 * max(1.0, np.abs(want).max()), g_["name"]
        worst = max(worst, _ratio(opt.p[sl], want, ref["p_bound"][sl]))
        assert torch.equal(g_["param"].detach().reshape(-1), opt.p[sl]), "the model's parameters are the arena's views"
    print(f"FusedSGD.original, one step of the tiny model: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    trained = {g_["name"] for g_ in opt.groups}
    frozen = [n for n, _ in cpu.named_parameters() if n not in trained]
    assert frozen and all(n.startswith("clip_encoder.") or n.startswith("backbone.") for n in frozen)


def test_original_schedule_after_the_step(dev, original_step):
    opt = original_step["opt"]
    k = (1 - 3 / 10) * (1 - 1e-6)                    # semivl.py:331-337 at iters = 3 < warmup_iters = 10
    lr = LR * (1 - k)
    assert opt.param_groups[0]["lr"] == lr and opt.param_groups[1]["lr"] == lr * LR_MULTI and len(opt.param_groups) == 2
    want = torch.tensor([(lr, lr * LR_MULTI)[g_["group"]] for g_ in opt.groups], dtype=torch.float32)
    assert torch.equal(opt.seg_lr.cpu(), want)
    opt.poly_lr(30, 50, warmup_iters=10)
    lr = LR * (1 - 30 / 50) ** 0.9
    assert [g["lr"] for g in opt.param_groups] == [lr, lr * LR_MULTI]
    want = torch.tensor([(lr, lr * LR_MULTI)[g_["group"]] for g_ in opt.groups], dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(opt.seg_lr.cpu(), want)
    assert {g_["group"] for g_ in opt.groups} == {0, 1}


def test_state_dict_resumes_bit_identically_and_interchanges_with_torch(dev):
    from semivl_amd.train import FusedSGD
    ha, z, c = _tiny(dev)
    hb, _, _ = _tiny(dev)
    oa, ob = FusedSGD.original(ha, LR, LR_MULTI, weight_decay=WD), FusedSGD.original(hb, LR, LR_MULTI, weight_decay=WD)
    assert FusedSGD.original(_tiny(dev)[0], LR, LR_MULTI, weight_decay=WD).state_dict()["state"] == {}       # no buffers before a step
    cpu, _, _ = _tiny()
    to = _reference_sgd(cpu, LR, LR_MULTI)
    named = dict(cpu.named_parameters())
    gen = torch.Generator().manual_seed(0)
    live = torch.zeros(oa.total)
    for i, g_ in enumerate(oa.groups):
        live[int(oa.seg_off[i]):int(oa.seg_off[i]) + g_["param"].numel()] = 1
    grads = [(torch.randn(oa.total, generator=gen) * 0.1 * live).to(dev) for _ in range(3)]
    for i in range(2):
        oa.g.copy_(grads[i]); oa.step(); oa.poly_lr(i + 1, 100)
        for g_ in oa.groups:
            named[g_["name"]].grad = g_["param"].main_grad.detach().cpu().clone()
        to.step()
        to.param_groups[0]["lr"], to.param_groups[1]["lr"] = oa.param_groups[0]["lr"], oa.param_groups[1]["lr"]
    sd, ts = oa.state_dict(), to.state_dict()
    # torch.optim.SGD's layout: two groups, params numbered through them, a momentum buffer per trained tensor only
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in ts["param_groups"]] and len(sd["param_groups"]) == 2
    assert sorted(sd["state"]) == sorted(ts["state"]) and len(sd["state"]) == len(oa.groups)
    for g, t in zip(sd["param_groups"], ts["param_groups"]):
        assert set(t) <= set(g), sorted(set(t) - set(g))
        assert all(g[k] == t[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov"))
    for j in ts["state"]:
        a, b = sd["state"][j]["momentum_buffer"], ts["state"][j]["momentum_buffer"]
        assert list(sd["state"][j]) == ["momentum_buffer"] and a.shape == b.shape
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), j
    # resume: fresh optimizer + load == uninterrupted, bit for bit
    ob.p.copy_(oa.p)
    ob.load_state_dict(sd)
    assert ob.step_count == 2 and torch.equal(ob.m, oa.m) and torch.equal(ob.seg_lr, oa.seg_lr)
    for o in (oa, ob):
        o.g.copy_(grads[2]); o.step()
    assert torch.equal(oa.p, ob.p) and torch.equal(oa.m, ob.m)
    # ours -> torch (the dict as it is), torch -> ours (no step_count / names in it)
    t2 = _reference_sgd(_tiny()[0], LR, LR_MULTI)
    t2.load_state_dict(sd)
    j0 = min(sd["state"])
    assert torch.equal(t2.state_dict()["state"][j0]["momentum_buffer"], sd["state"][j0]["momentum_buffer"])
    assert t2.param_groups[1]["lr"] == sd["param_groups"][1]["lr"]
    o3 = FusedSGD.original(_tiny(dev)[0], LR, LR_MULTI, weight_decay=WD)
    o3.load_state_dict(ts)
    assert o3.step_count >= 1 and o3.param_groups[0]["lr"] == ts["param_groups"][0]["lr"]
    slot = dict(o3.all_params)
    names = sd["names"]
    for j in ts["state"]:
        ai = slot[names[j]]
        off, cnt = int(o3.seg_off[ai]), o3.groups[ai]["param"].numel()
        assert torch.equal(o3.m[off:off + cnt].cpu().view(ts["state"][j]["momentum_buffer"].shape), ts["state"][j]["momentum_buffer"])
    assert torch.equal(o3.seg_lr, oa.seg_lr)


def test_type_sgd_through_build_optimizer(dev):
    """cfg['optimizer'] = dict(type='SGD', ...) with exp 40's custom keys: per-tensor lr / weight decay as mmcv_param_groups
    says, nesterov momentum, one training step inside the bound."""
    from semivl_amd.synthetic import exp40_cfg
    from semivl_amd.train import FusedSGD, build_optimizer, mmcv_param_groups
    ck = exp40_cfg()["optimizer"]["paramwise_cfg"]["custom_keys"]
    hip, z, c = _tiny(dev)
    lr, wd = R.f32(0.01), R.f32(5e-4)
    opt = build_optimizer(hip, dict(type="SGD", lr=lr, momentum=R.MOM, weight_decay=wd, nesterov=True,
                                    paramwise_cfg=dict(custom_keys=ck)))
    assert isinstance(opt, FusedSGD) and opt.nesterov and opt.param_groups is opt.groups
    named = [(n, p) for n, p in hip.named_parameters() if p.requires_grad and not n.startswith("clip_encoder.")]
    want = mmcv_param_groups(named, lr, wd, ck)
    assert [g["name"] for g in want] == [g["name"] for g in opt.groups]
    assert torch.equal(opt.seg_lr.cpu(), torch.tensor([g["lr"] for g in want], dtype=torch.float32))
    assert torch.equal(opt.seg_wd.cpu(), torch.tensor([g["weight_decay"] for g in want], dtype=torch.float32))
    assert len({g["lr"] for g in want}) >= 2                    # the keys really bite (backbone x 0.01, head x 10)
    p0 = opt.p.clone()
    opt._applied_lr = opt.seg_lr.clone()
    _train_step(hip, z, c, dev, opt, 3, 50)
    ref = _arena_ref(opt, p0, 1)
    worst = max(_ratio(opt.p, ref["p"], ref["p_bound"]), _ratio(opt.m, ref["m"], ref["m_bound"]))
    print(f"FusedSGD(type='SGD', nesterov), one step of the tiny model: worst error / bound = {worst:.3f}")
    assert worst <= 1.0 and not torch.equal(opt.p, p0)
    assert abs(opt.groups[0]["lr"] - opt.groups[0]["initial_lr"] * (1 - 3 / 50) ** 0.9) < 1e-15
    sd = opt.state_dict()
    nall = len(list(hip.named_parameters()))
    assert [g["params"] for g in sd["param_groups"]] == [[j] for j in range(nall)] and len(sd["state"]) == len(opt.groups)
    assert all("momentum_buffer" in s for s in sd["state"].values()) and sd["param_groups"][0]["nesterov"] is True
    o2 = build_optimizer(_tiny(dev)[0], dict(type="SGD", lr=lr, momentum=R.MOM, weight_decay=wd, nesterov=True,
                                             paramwise_cfg=dict(custom_keys=ck)))
    o2.load_state_dict(sd)
    assert torch.equal(o2.m, opt.m) and torch.equal(o2.seg_lr, opt.seg_lr) and o2.step_count == 1


def test_grad_all_reducer_scales_the_sgd_step(dev):
    """GradAllReducer(FusedSGD) with the world = 2 / injected-collective hooks: 'SUM over two ranks holding the same
    gradient' = x2 on the communication stream, grad_scale = 1 / 2 reaches the kernel: the update is the one sgd_ref gives
    for gscale = 0.5 on the summed gradient, and equals the single-process step bit for bit (x2 and x1/2 are exact)."""
    from semivl_amd.train import FusedSGD, GradAllReducer

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

    res = []
    for with_reducer in (False, True):
        hip, z, c = _tiny(dev)
        opt = FusedSGD.original(hip, LR, LR_MULTI, weight_decay=WD)
        red = GradAllReducer(opt, bucket_mb=0.25, world=2, collective=two_identical_ranks) if with_reducer else None
        p0 = opt.p.clone()
        opt._applied_lr = opt.seg_lr.clone()
        _train_step(hip, z, c, dev, opt, 0, 10, red=red)
        torch.cuda.synchronize()
        res.append((opt.p.clone(), opt.g.clone()))
        if red is not None:
            assert opt.grad_scale == 0.5 and len(calls) == len(red.buckets) >= 2
            ref = _arena_ref(opt, p0, 1, gscale=0.5)
            worst = _ratio(opt.p, ref["p"], ref["p_bound"])
            print(f"GradAllReducer(FusedSGD), world = 2: worst error / bound = {worst:.3f}")
            assert worst <= 1.0
    assert torch.equal(res[1][1], 2.0 * res[0][1]), "the arena holds the sum over the two ranks"
    assert torch.equal(res[0][0], res[1][0])
