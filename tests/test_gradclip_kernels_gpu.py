"""svl_grad_clip_f32 on the GPU against its float64 restatement (tests/gradclip_ref.py, proven on the CPU by
tests/test_gradclip_ref.py) with the a-priori bound |out - ref| <= (2^-24 + n 2^-52) |ref|, and the device-scale step entry
points (svl_adamw_step_dscale, svl_sgd_step_dscale) bit for bit against the plain ones.  The worst error / bound ratio of
every case is printed (-s)."""
import math

import pytest
import torch

import gradclip_ref as R
import sgd_ref as S
from small_kernel_ref import SENTINEL, guard_intact, guarded

pytestmark = pytest.mark.gpu

ONE_PASS = 1024 * 256 * 4                  # floats one trip of the capped grid covers (csrc/gradclip.hip: GC_GRID_CAP x GC_TRIP)
RAGGED = [7, 1, 130, 33, 4, 1025, 2]       # a multi-segment arena from arena_layout: padding zeros inside
TOTALS = [1, 3, 4, 5, 1023, 1024, 1025, "ragged", 2 * ONE_PASS + 5]
GUARD = 64


def _values(kind, total, seed):
    """(arena, number of live elements): `total` values of the range, or the RAGGED tensors laid out by arena_layout."""
    if total != "ragged":
        return R.values(kind, total, seed), total
    from semivl_amd.optim import arena_layout
    offs, n = arena_layout(RAGGED)
    flat = R.values(kind, sum(RAGGED), seed)
    g = torch.zeros(n)
    for o, t in zip(offs, flat.split(RAGGED)):
        g[o:o + t.numel()] = t
    assert n % 4 == 0 and n > sum(RAGGED)
    return g, n


def _run(dev, g, max_norm, norm_type, gscale):
    """stats (CPU, float64) of one guarded call; checks the guard bands of ws and stats and that ws was written in full."""
    from semivl_amd import lib as L
    from semivl_amd import ops
    nws = int(L.load().svl_grad_clip_ws_doubles(g.numel()))
    wb, ws = guarded(nws, torch.float64, dev, guard=GUARD)
    sb, stats = guarded(4, torch.float32, dev, guard=GUARD)
    out = ops.grad_clip(g, max_norm, norm_type, gscale=gscale, stats=stats, ws=ws)
    assert out is stats
    assert guard_intact(wb, nws, guard=GUARD) and guard_intact(sb, 4, guard=GUARD), "guard bands written"
    assert not (ws == SENTINEL).any(), "a block left its partial unwritten"
    return stats.clone()


def _check(got, g_cpu, n, max_norm, norm_type, gscale, strict_relative=True):
    """Worst |stats[k] - ref| / bound over k = 0..2 (0.0 for the non-finite cases, which must match exactly); the flag is
    exact."""
    ref = R.clip_ref(g_cpu, max_norm, norm_type, gscale)
    got = [float(v) for v in got.double().cpu()]
    assert got[3] == (1.0 if ref[3] else 0.0), (got, ref)
    worst = 0.0
    for k in range(3):
        if math.isnan(ref[k]):
            assert math.isnan(got[k]), (k, got, ref)
        elif math.isinf(ref[k]) or ref[k] == 0.0:
            assert got[k] == ref[k], (k, got, ref)
        else:
            b = R.relative_bound(ref[k], n) if strict_relative else R.bound(ref[k], n)
            worst = max(worst, abs(got[k] - ref[k]) / b)
    return worst


def _max_norm_for(kind, g_cpu, norm_type, gscale):
    """A live clip for the normal and the huge range: half the norm (an fp32 number); 1.0 for the others (zeros and tiny
    stay unclipped: coef = 1 exactly; NaN / inf decide the coefficient themselves)."""
    if kind not in ("normal", "huge"):
        return 1.0
    return R.f32(0.5 * R.clip_ref(g_cpu, math.inf, norm_type, gscale)[0])


@pytest.mark.parametrize("norm_type", [2.0, "inf"], ids=["l2", "max"])
@pytest.mark.parametrize("kind", R.RANGES)
def test_grad_clip_within_bound(dev, kind, norm_type):
    """Every total x this value range: aligned and 4 bytes off a 16-byte boundary (the scalar path; the same bits, because
    which lane reads which element depends on the total alone), twice (bit for bit), and `tiny` both as it is (the norm is a
    subnormal fp32 number: rounded to a multiple of 2^-149, R.bound) and lifted by gscale = 2^20 into the normal range,
    where the relative bound applies as stated."""
    worst = 0.0
    for ti, total in enumerate(TOTALS):
        g_cpu, n = _values(kind, total, seed=20 + ti)
        off = torch.empty(n + 4, device=dev)                 # torch's allocations are 256-byte aligned
        g, g_off = g_cpu.to(dev), off[1:1 + n]
        g_off.copy_(g_cpu)
        assert g.data_ptr() % 16 == 0 and g_off.data_ptr() % 16 == 4
        scales = [1.0, 2.0 ** 20] if kind == "tiny" else [R.f32(1.0 / 3.0) if ti % 2 else 1.0]
        for gscale in scales:
            max_norm = _max_norm_for(kind, g_cpu, norm_type, gscale)
            a = _run(dev, g, max_norm, norm_type, gscale)
            b = _run(dev, g, max_norm, norm_type, gscale)
            c = _run(dev, g_off, max_norm, norm_type, gscale)
            same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
            assert same(a, b), "two runs differ"
            assert same(a, c), "the scalar path does not reproduce the 16-byte path"
            subnormal = kind == "tiny" and gscale == 1.0
            r = _check(a, g_cpu, n, max_norm, norm_type, gscale, strict_relative=not subnormal)
            if kind in ("normal", "huge"):
                assert float(a[1]) < 1.0, "the clip was meant to be live"
            if kind in ("zeros", "tiny"):
                assert float(a[1]) == 1.0 and float(a[2]) == gscale
            worst = max(worst, r)
    print(f"svl_grad_clip_f32 {kind}/{norm_type}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_grad_clip_reports_only_with_an_infinite_max_norm(dev):
    from semivl_amd import ops
    g_cpu = R.values("normal", 1025, 3)
    for nt in (2.0, "inf"):
        st = ops.grad_clip(g_cpu.to(dev), math.inf, nt, gscale=0.25)
        assert float(st[1]) == 1.0 and float(st[2]) == 0.25 and float(st[3]) == 0.0
        assert _check(st, g_cpu, 1025, math.inf, nt, 0.25) <= 1.0
    st = ops.grad_clip(g_cpu.to(dev), math.inf, "inf")
    assert float(st[0]) == float(g_cpu.abs().max()), "the max norm is exact"


def test_grad_clip_workspace_query_and_refusals(dev):
    from semivl_amd import lib as L
    from semivl_amd import ops
    lib = L.load()
    q = lib.svl_grad_clip_ws_doubles
    assert [q(t) for t in (-1, 0, 1, 1024, 1025, ONE_PASS, ONE_PASS + 1, 2 * ONE_PASS + 5, 118_000_000)] == \
        [0, 0, 1, 1, 2, 1024, 1024, 1024, 1024]
    g = torch.ones(8, device=dev)
    ws = torch.empty(1, dtype=torch.float64, device=dev)
    stats = torch.full((4,), SENTINEL, device=dev)

    def status(g_=g, total=8, kind=0, gscale=1.0, max_norm=1.0, ws_=ws, stats_=stats):
        return lib.svl_grad_clip_f32(ops._p(g_), total, kind, gscale, max_norm, ops._p(ws_), ops._p(stats_), ops._st())

    bad = [dict(gscale=0.0), dict(gscale=-1.0), dict(gscale=math.inf), dict(gscale=math.nan), dict(max_norm=0.0),
           dict(max_norm=-1.0), dict(max_norm=math.nan), dict(g_=None), dict(ws_=None), dict(stats_=None), dict(total=0),
           dict(kind=2)]
    for kw in bad:
        assert status(**kw) == -1 and "svl_grad_clip_f32" in L.last_error(), kw
    torch.cuda.synchronize()
    assert bool((stats == SENTINEL).all()), "a refused call wrote"
    with pytest.raises(RuntimeError, match="svl_grad_clip_f32"):
        ops.grad_clip(g, -1.0)
    with pytest.raises(NotImplementedError, match="norm_type"):
        ops.grad_clip(g, 1.0, norm_type=1.0)
    assert status(max_norm=math.inf) == 0 and status() == 0
    torch.cuda.synchronize()
    assert _check(stats, torch.ones(8), 8, 1.0, 2.0, 1.0) <= 1.0
    # the device-scale steps refuse a null scale like any other null pointer
    case = S.arena([8], 1)
    p, gr, m = case["p"].to(dev), case["gs"][0].to(dev), torch.zeros(8, device=dev)
    keep = [case[k].to(dev) for k in ("seg_off", "seg_lr", "seg_wd")]
    tabs = [ops._p(t) for t in keep]
    rc = lib.svl_sgd_step_dscale(ops._p(p), ops._p(gr), ops._p(m), *tabs, 1, 8, 0.9, 0.0, 0, 1, None, None, 0.0, ops._st())
    assert rc == -1 and "svl_sgd_step_dscale" in L.last_error()
    rc = lib.svl_adamw_step_dscale(ops._p(p), ops._p(gr), ops._p(m), ops._p(m), *tabs, 1, 8, 0.9, 0.999, 1e-8, 1, None, None,
                                   0.0, ops._st())
    assert rc == -1 and "svl_adamw_step_dscale" in L.last_error()


# ------------------------------------------------------------------------------------------------ device-scale steps
SCALE = R.f32(0.37)                 # an fp32 number with a full mantissa: the host float and the device float are the same value
BIG = [1500001, 3, 2 * 2048 * 256 * 4 + 77, 5]      # beyond two passes of either step kernel's capped grid


def _both(dev, run, tensors):
    """`run(gscale=..., gscale_dev=...)` three steps from the same state in both forms; every tensor bit-equal after each."""
    sdev = torch.tensor([SCALE], dtype=torch.float32, device=dev)
    start = [t.clone() for t in tensors]
    trace = []
    for form in ("plain", "dscale"):
        for t, s in zip(tensors, start):
            t.copy_(s)
        steps = []
        for step in (1, 2, 3):
            run(step, **(dict(gscale=SCALE) if form == "plain" else dict(gscale_dev=sdev)))
            steps.append([t.clone() for t in tensors])
        trace.append(steps)
    for step, (a, b) in enumerate(zip(*trace), 1):
        for k, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (step, k)
    assert not torch.equal(trace[0][2][0], start[0])
    assert float(sdev[0]) == SCALE


def _sgd_both(dev, sizes, mode, with_ema):
    from semivl_amd import ops
    case = S.arena(sizes, 31)
    md, n = S.MODES[mode], case["total"]
    gen = torch.Generator().manual_seed(32)
    p, m = case["p"].to(dev), torch.zeros(n, device=dev)
    e = (torch.randn(n, generator=gen) * ~case["pad"]).to(dev)
    gs = [g.to(dev) for g in case["gs"]]
    tabs = [case[k].to(dev) for k in ("seg_off", "seg_lr", "seg_wd")]
    has_m = md["momentum"] != 0

    def run(step, **scale):
        ops.sgd_step(p, gs[step - 1], m if has_m else None, *tabs, case["nseg"], md["momentum"], md["dampening"],
                     md["nesterov"], step, ema=e if with_ema else None, ema_decay=0.99, **scale)
    _both(dev, run, [p, m, e])


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("mode", ["no_momentum", "momentum", "dampening", "nesterov"])
def test_sgd_step_dscale_equals_the_plain_entry_point(dev, mode, with_ema):
    """svl_sgd_step_dscale against svl_sgd_step: no momentum, momentum (its first step clones the gradient, steps 2 and 3
    do not), dampening, nesterov; with and without the EMA teacher."""
    _sgd_both(dev, S.SIZES["ragged"], mode, with_ema)


@pytest.mark.parametrize("mode,with_ema", [("nesterov", True), ("no_momentum", False)])
def test_sgd_step_dscale_beyond_one_pass_of_the_grid(dev, mode, with_ema):
    _sgd_both(dev, BIG, mode, with_ema)


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("sizes", ["ragged", "big"])
def test_adamw_step_dscale_equals_the_plain_entry_point(dev, sizes, with_ema):
    from semivl_amd import ops
    case = S.arena(S.SIZES["ragged"] if sizes == "ragged" else BIG, 33)
    n = case["total"]
    gen = torch.Generator().manual_seed(34)
    p, m, v = case["p"].to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    e = (torch.randn(n, generator=gen) * ~case["pad"]).to(dev)
    gs = [g.to(dev) for g in case["gs"]]
    tabs = [case[k].to(dev) for k in ("seg_off", "seg_lr", "seg_wd")]

    def run(step, **scale):
        ops.adamw_step(p, gs[step - 1], m, v, *tabs, case["nseg"], 0.9, 0.999, 1e-8, step, ema=e if with_ema else None,
                       ema_decay=0.99, **scale)
    _both(dev, run, [p, m, v, e])


def test_the_scale_is_read_when_the_kernel_runs(dev):
    """The *_dscale kernels read the scale from the device: a value written by an EARLIER launch on the stream (here
    grad_clip's stats[2]) is the one applied, with no host round trip in between."""
    from semivl_amd import ops
    case = S.arena([1025, 7], 35)
    n = case["total"]
    g = case["gs"][0].to(dev)
    tabs = [case[k].to(dev) for k in ("seg_off", "seg_lr", "seg_wd")]
    norm = R.clip_ref(case["gs"][0], math.inf)[0]
    stats = ops.zeros(4, device=dev)
    p1 = case["p"].to(dev)
    ops.grad_clip(g, R.f32(0.5 * norm), stats=stats)
    ops.sgd_step(p1, g, None, *tabs, case["nseg"], 0.0, 0.0, False, 1, gscale_dev=stats[2:3])
    scale = float(stats[2])
    assert 0.49 < scale < 0.51
    p2 = case["p"].to(dev)
    ops.sgd_step(p2, g, None, *tabs, case["nseg"], 0.0, 0.0, False, 1, gscale=scale)
    assert torch.equal(p1, p2)
    with pytest.raises(AssertionError):
        ops.sgd_step(p2, g, None, *tabs, case["nseg"], 0.0, 0.0, False, 1, gscale_dev=stats)      # four floats, not one
