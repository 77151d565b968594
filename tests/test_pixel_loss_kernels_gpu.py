"""GPU: the unlabelled pixel-loss and label kernels (svl_ce_fused_f32, svl_ce_up_fused_f32, svl_softmax_max_f32,
svl_softmax_max_up_f32, svl_maskclip_labels, svl_concept_max_f32, svl_cutmix_f32 / _i64, svl_count_valid_i64) against the
float64 restatements of tests/pixel_loss_ref.py, inside the limits derived there from the kernels' operation counts
(tests/test_pixel_loss_ref.py holds the restatements to torch's float64, torch's fp32 to the same limits, and shows that the
limits see each of a list of faults).  Error / limit is printed (-s); the last test prints the largest per kernel.

Every output sits between guard bands of NaN (labels: of -7, on a -7 background): every element is written, nothing else is.
Labels of the resized forms are compared where the float64 top-2 gap exceeds twice the bound on an interpolated logit
(MaskCLIP: and |conf - thresh| exceeds the bound on conf); on every random case that excuses at most 1 % of the pixels, and
constructed ties (a constant map, two bit-identical planes) are not excused at all: the first index wins.

Geometries of the resize-fused kernels (pixel_loss_ref.UP_GEOMS, chosen with the host-only queries svl_ce_up_num_blocks /
svl_ce_up_lsw_num_blocks): which edge each one hits is written next to it there; test_geometry_queries asserts what the
queries answer for them, for the refused ones, and that N = 257 is refused by svl_ce_num_blocks and the entry point."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import pixel_loss_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL = -7
ONE_PASS = 4096 * 256          # threads of the capped grid (grid_for: at most 4096 blocks of 256)
WORST = {}


def note(kernel, value):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(value))


def guarded(shape, dev, dtype=torch.float32):
    n = int(np.prod(shape))
    fill = SENTINEL if dtype == torch.int64 else float("nan")
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    if buf.dtype == torch.int64:
        return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()) and \
            not bool((buf[GUARD:-GUARD] == SENTINEL).any())
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()) and \
        not bool(torch.isnan(buf[GUARD:-GUARD]).any())


def _B(N):
    return 1 if N >= 100 else 2


@functools.lru_cache(None)
def fused_inputs(B, N, HW, case):
    return R.case_inputs(case, (B, N, HW), (B, HW), seed=101)


@functools.lru_cache(None)
def up_inputs(geom, case):
    N, h, w, H, W = geom
    return R.case_inputs(case, (_B(N), N, h, w), (_B(N), H, W), seed=102)


def on(dev, kw):
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in kw.items()}


def run_ce(dev, xd, td, dkw, gs, up=None, grad=True):
    """One guarded launch of the full-resolution (up = None) or the resize-fused kernel -> (dlogits or None, sums)."""
    from semivl_amd import ops
    dbuf, dl = guarded(tuple(xd.shape), dev) if grad else (None, None)
    sbuf, sums = guarded((4,), dev, torch.float64)
    if up is None:
        ops.ce_fused(xd, td, dlogits=dl, gscale=gs if grad else None, sums_out=sums, **dkw)
    else:
        ops.ce_up_fused(xd, up[0], up[1], up[2], td, dlogits=dl, gscale=gs if grad else None, sums_out=sums, **dkw)
    torch.cuda.synchronize()
    assert guards_intact(sbuf) and (dbuf is None or guards_intact(dbuf))
    return dl, sums


def check_ce(dev, kernel, label, x, t, kw, g, up=None):
    if up is None:
        ref = R.ce_plain(x, t, g=g, **kw)
        bnd = R.ce_bounds(ref)
    else:
        ref = R.ce_plain_up(x, up[0], up[1], up[2], t, g=g, **kw)
        bnd = R.ce_bounds(ref, (x, *up))
    xd, td, dkw = x.to(dev), t.to(dev), on(dev, kw)
    gs = torch.tensor(g, dtype=torch.float32, device=dev)
    dl, sums = run_ce(dev, xd, td, dkw, gs, up)
    r = R.ce_ratios(sums, dl, ref, bnd)
    print(f"\n[{kernel} {label}] error / limit: " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    for k, v in r.items():
        note(f"{kernel} {'sums' if k.startswith('sum') else k}", v)
    assert max(r.values()) <= 1.0, r
    assert sums[3].item() == ref["sums"][3].item() == float(int(ref["sums"][3].item()))
    # pixels (cells) that no scale reaches hold exact zeros
    G = ref["gt"] + ref["gm"]
    if up is None:
        dead = (G == 0).unsqueeze(1).expand_as(ref["grad"])
    else:
        dead = (R.transpose_plus(G, x.shape[2], x.shape[3], up[2]) == 0).unsqueeze(1).expand_as(ref["grad"])
    assert bool((dl.cpu()[dead] == 0).all())
    # two runs, bit for bit; the forward-only call returns the same sums
    dl2, s2 = run_ce(dev, xd, td, dkw, gs, up)
    _, s3 = run_ce(dev, xd, td, dkw, gs, up, grad=False)
    assert torch.equal(dl2, dl) and torch.equal(s2, sums) and torch.equal(s3, sums)
    return ref, bnd, dl, sums, (xd, td, dkw, gs)


# ------------------------------------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("case,form", R.case_forms())
@pytest.mark.parametrize("B,N,HW", R.FUSED_SHAPES)
def test_ce_fused(dev, B, N, HW, case, form):
    x, m = fused_inputs(B, N, HW, case)
    t, kw = R.form_kwargs(form, m, B)
    check_ce(dev, "svl_ce_fused_f32", f"B{B} N{N} HW{HW} {case} {form}", x, t, kw, R.form_gscale(form, B * HW))


@pytest.mark.parametrize("case,form", R.case_forms())
@pytest.mark.parametrize("geom,align", R.up_pairs())
def test_ce_up_fused(dev, geom, align, case, form):
    from semivl_amd import ops
    N, h, w, H, W = geom
    B = _B(N)
    assert ops.ce_up_ok(B, N, h, w, H, W, align)
    x, m = up_inputs(geom, case)
    t, kw = R.form_kwargs(form, m, B)
    up = (H, W, align)
    ref, bnd, dl, sums, (xd, td, dkw, gs) = check_ce(dev, "svl_ce_up_fused_f32", f"{geom} align={align} {case} {form}", x, t, kw,
                                                     R.form_gscale(form, B * H * W), up)
    # the full-resolution kernel on svl_bilinear_planes_fwd's output: both lie within the resized form's limits of the
    # float64 reference (they contain the interpolation's own error and more roundings than the two-pass kernel makes)
    full = ops.bilinear_planes_fwd(xd, h, w, align, H, W)
    dfull = torch.full_like(full, float("nan"))
    sf = ops.ce_fused(full, td, dlogits=dfull, gscale=gs, **dkw)
    dlf = ops.bilinear_planes_bwd(dfull, h, w, align, H, W)
    rs = [R.ratio((sf.cpu()[k] - sums.cpu()[k]).abs(), 2 * bnd["sums"][k]) for k in range(3)]
    rg = R.ratio((dlf.double().cpu() - dl.double().cpu()).abs(), 2 * bnd["grad"])
    print(f"   against the unfused kernels, difference / sum of limits: sums {max(rs):.4f}, gradient {rg:.4f}")
    assert max(rs) <= 1.0 and rg <= 1.0 and sf[3].item() == sums[3].item()


def _all_ignored(dev, x, t, up):
    xd = x.to(dev)
    td = torch.full(t.shape, 255, dtype=torch.int64, device=dev)
    gs = torch.tensor([float("inf"), 0.0], device=dev)
    dl, sums = run_ce(dev, xd, td, dict(use_ignore_t=True), gs, up)
    assert bool((dl == 0).all()) and sums.tolist() == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("B,N,HW", R.FUSED_SHAPES)
def test_every_target_ignored_and_an_infinite_scale_full(dev, B, N, HW):
    x, m = fused_inputs(B, N, HW, "baseline")
    _all_ignored(dev, x, m["target"], None)


@pytest.mark.parametrize("geom,align", R.up_pairs())
def test_every_target_ignored_and_an_infinite_scale_up(dev, geom, align):
    x, m = up_inputs(geom, "baseline")
    _all_ignored(dev, x, m["target"], (geom[3], geom[4], align))


def test_labels_outside_the_classes_read_no_logit_in_both_forms(dev):
    """254, and 255 with use_ignore_t = 0, at N = 21 (target and guidance map): lse - 0 and no one-hot term, the same in the
    full-resolution kernel (which used to read LDS outside its tile there) and the resize-fused one."""
    x, m = fused_inputs(2, 21, 672, "baseline")
    t, mc = m["lab"].clone(), m["mc"].clone()
    t[0, ::3] = 254
    t[1, 1::4] = 255
    mc[0, 1::5] = 254
    kw = dict(use_ignore_t=False, conf=m["conf"], ign=m["ign"], conf_thresh=0.0, mc=mc)
    ref = check_ce(dev, "svl_ce_fused_f32", "labels 254 / 255", x, t, kw, (R.f32(1e-3), R.f32(3e-4)))[0]
    assert ref["sums"][0].item() > 0 and bool((t >= 21).any())
    geom = (21, 8, 8, 32, 32)
    xu, mu = up_inputs(geom, "baseline")
    t, mc = mu["lab"].clone(), mu["mc"].clone()
    t[0, ::3] = 254
    t[1, :, 1::4] = 255
    mc[0, 1::5] = 254
    kw = dict(use_ignore_t=False, conf=mu["conf"], ign=mu["ign"], conf_thresh=0.0, mc=mc)
    for align in (False, True):
        check_ce(dev, "svl_ce_up_fused_f32", f"labels 254 / 255 align={align}", xu, t, kw, (R.f32(1e-3), R.f32(3e-4)), (32, 32, align))


def test_img_weight_without_conf_is_refused_by_name(dev):
    from semivl_amd import lib as L
    from semivl_amd import ops
    x, m = fused_inputs(2, 21, 672, "baseline")
    iw = torch.tensor([0.25, 0.75], device=dev)
    with pytest.raises(RuntimeError, match="img_weight"):
        ops.ce_fused(x.to(dev), m["target"].to(dev), True, img_weight=iw)
    assert "img_weight" in L.last_error() and "svl_ce_fused_f32" in L.last_error()
    xu, mu = up_inputs((5, 8, 8, 32, 32), "baseline")
    with pytest.raises(RuntimeError, match="img_weight"):
        ops.ce_up_fused(xu.to(dev), 32, 32, False, mu["target"].to(dev), True, img_weight=iw)
    assert "img_weight" in L.last_error() and "svl_ce_up_fused_f32" in L.last_error()


def _up_entry_status(dev, N, h, w, H, W, align):
    """Status of svl_ce_up_fused_f32 itself (ops.ce_up_fused asks the query first) on a geometry; nothing is launched when it
    refuses."""
    from semivl_amd import lib as L
    from semivl_amd import ops
    x = torch.zeros(1, N, h, w, device=dev)
    t = torch.zeros(1, H, W, dtype=torch.int64, device=dev)
    part = torch.zeros(64, 4, device=dev)
    d = L.CeUpDesc(ops._p(x), 1, N, h, w, H, W, 1 if align else 0, ops._p(t), 1, None, None, 0.0, 0, None, ops._p(part), None, None,
                   None)
    return L.load().svl_ce_up_fused_f32(C.byref(d), ops._st())


def test_geometry_queries(dev):
    from semivl_amd import lib as L
    from semivl_amd import ops
    lib = L.load()
    for g in R.UP_GEOMS:
        for align in (False, True):
            want = R.UP_ONLY_ALIGN.get(g, align) == align
            assert (lib.svl_ce_up_num_blocks(2, *g, int(align)) > 0) == want, (g, align)
            assert (lib.svl_ce_up_lsw_num_blocks(2, *g, int(align)) > 0) == want, (g, align)
    for *g, align in R.UP_REFUSED:
        assert lib.svl_ce_up_num_blocks(2, *g, int(align)) == -1 and lib.svl_ce_up_lsw_num_blocks(2, *g, int(align)) == -1, g
        assert _up_entry_status(dev, *g, align) == -1 and "unsupported geometry" in L.last_error()
        with pytest.raises(RuntimeError, match="unsupported geometry"):
            ops.softmax_max_up(torch.zeros(1, *g[:3], device=dev), g[3], g[4], align)
    # N = 256 is the last class count of the full-resolution kernel
    assert lib.svl_ce_num_blocks(1, 256, 70) == 2 and lib.svl_ce_num_blocks(1, 257, 70) == -1
    x = torch.zeros(1, 257, 70, device=dev)
    t = torch.zeros(1, 70, dtype=torch.int64, device=dev)
    part = torch.zeros(8, 4, device=dev)
    d = L.CeDesc(ops._p(x), 1, 257, 70, ops._p(t), 1, None, None, 0.0, 0, None, ops._p(part), None, None, None)
    assert lib.svl_ce_fused_f32(C.byref(d), ops._st()) == -1
    assert "svl_ce_fused_f32" in L.last_error() and "N=257" in L.last_error()


# ------------------------------------------------------------------------------------------------ softmax-max
def run_softmax_max(dev, xd, up=None):
    from semivl_amd import lib as L
    from semivl_amd import ops
    B, N = xd.shape[:2]
    shape = (B, *xd.shape[2:]) if up is None else (B, up[0], up[1])
    cbuf, conf = guarded(shape, dev)
    lbuf, lab = guarded(shape, dev, torch.int64)
    if up is None:
        L.check(L.load().svl_softmax_max_f32(ops._p(xd), B, N, xd[0, 0].numel(), ops._p(conf), ops._p(lab), ops._st()))
    else:
        L.check(L.load().svl_softmax_max_up_f32(ops._p(xd), B, N, xd.shape[2], xd.shape[3], up[0], up[1], 1 if up[2] else 0,
                                                ops._p(conf), ops._p(lab), ops._st()))
    torch.cuda.synchronize()
    assert guards_intact(cbuf) and guards_intact(lbuf)
    return conf, lab


def check_softmax_max(dev, kernel, label, x, case, up=None):
    if up is None:
        conf, lab, gap = R.softmax_max(x)
        delta, full = None, x
    else:
        conf, lab, gap = R.softmax_max_up(x, *up)
        delta, full = R.interp_bound(x, *up)[0], R.resize(x, *up)
    got_c, got_l = run_softmax_max(dev, x.to(dev), up)
    r = R.ratio((got_c.double().cpu() - conf).abs(), R.conf_bound(full, delta))
    if case in ("equal", "twin"):      # a constructed tie: nothing excused, and the exact answer is the first index (the float64
        clear = torch.ones_like(lab, dtype=torch.bool)      # resize of two equal planes need not be equal to the last bit)
        lab = torch.full_like(lab, R.tie_first(case, x.shape[1]))
    elif up is None:                   # exact comparisons of the inputs: nothing excused
        clear = torch.ones_like(lab, dtype=torch.bool)
    else:
        clear = gap > 2 * delta
        assert 1.0 - clear.double().mean().item() <= 0.01
    print(f"\n[{kernel} {label}] conf error / limit {r:.4f}; labels compared {clear.double().mean().item():.4f}")
    note(f"{kernel} conf", r)
    assert r <= 1.0
    assert torch.equal(got_l.cpu()[clear], lab[clear])


@pytest.mark.parametrize("case", R.VALUE_CASES)
@pytest.mark.parametrize("B,N,HW", R.FUSED_SHAPES)
def test_softmax_max(dev, B, N, HW, case):
    check_softmax_max(dev, "svl_softmax_max_f32", f"B{B} N{N} HW{HW} {case}", fused_inputs(B, N, HW, case)[0], case)


@pytest.mark.parametrize("case", R.VALUE_CASES)
@pytest.mark.parametrize("geom,align", R.up_pairs())
def test_softmax_max_up(dev, geom, align, case):
    check_softmax_max(dev, "svl_softmax_max_up_f32", f"{geom} align={align} {case}", up_inputs(geom, case)[0], case,
                      (geom[3], geom[4], align))


# ------------------------------------------------------------------------------------------------ the sweep
def sweep_outs(lib, n_in, align, rows):
    """The `out` sizes of one `in`: the listed ones and the largest the query accepts; then that + 1, which it refuses."""
    def ok(o):
        g = (n_in, 3, o, 5) if rows else (3, n_in, 5, o)
        return lib.svl_ce_up_num_blocks(1, 2, *g, int(align)) > 0
    largest = max(o for o in range(n_in, 6 * n_in + 2) if ok(o))
    assert not ok(largest + 1)
    cand = {n_in, n_in + 1, 2 * n_in - 1, 2 * n_in, 2 * n_in + 1, 3 * n_in, 4 * n_in, int(4.5 * n_in), largest}
    return sorted(o for o in cand if ok(o)), largest


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("n_in", list(range(2, 20)) + [24, 25])
def test_sweep(dev, n_in, align):
    """B = 1, N = 2: every accepted size of the list on the row axis with a fixed 3 -> 5 column axis, then swapped: softmax-max
    writes every pixel once and agrees with float64, the supervised cross entropy counts every pixel once, its loss and its
    head-resolution gradient lie inside the limits; one past the largest size is refused by the query and the entry points."""
    from semivl_amd import lib as L
    from semivl_amd import ops
    lib = L.load()
    g_ = torch.Generator().manual_seed(1000 + n_in)
    worst = 0.0
    for rows in (True, False):
        outs, largest = sweep_outs(lib, n_in, align, rows)
        assert largest in outs
        bad = (2, n_in, 3, largest + 1, 5) if rows else (2, 3, n_in, 5, largest + 1)
        assert _up_entry_status(dev, *bad, align) == -1 and "unsupported geometry" in L.last_error()
        with pytest.raises(RuntimeError, match="unsupported geometry"):
            ops.softmax_max_up(torch.zeros(1, *bad[:3], device=dev), bad[3], bad[4], align)
        for o in outs:
            h, w, H, W = (n_in, 3, o, 5) if rows else (3, n_in, 5, o)
            x = torch.randn(1, 2, h, w, generator=g_) * 2
            t = torch.randint(0, 2, (1, H, W), generator=g_)
            up = (H, W, align)
            conf, lab, gap = R.softmax_max_up(x, *up)
            delta = R.interp_bound(x, *up)[0]
            gc, gl = run_softmax_max(dev, x.to(dev), up)
            clear = gap > 2 * delta
            rc = R.ratio((gc.double().cpu() - conf).abs(), R.conf_bound(R.resize(x, *up), delta))
            assert rc <= 1.0 and torch.equal(gl.cpu()[clear], lab[clear]), (h, w, H, W)
            g = (R.f32(1.0 / (H * W)), 0.0)
            ref = R.ce_plain_up(x, H, W, align, t, use_ignore_t=True, g=g)
            bnd = R.ce_bounds(ref, (x, *up))
            dl, sums = run_ce(dev, x.to(dev), t.to(dev), dict(use_ignore_t=True), torch.tensor(g, device=dev), up)
            r = R.ce_ratios(sums, dl, ref, bnd)
            assert sums[3].item() == H * W and max(r.values()) <= 1.0, ((h, w, H, W), r)
            worst = max(worst, rc, max(r.values()))
    note("sweep (both kernels)", worst)
    print(f"\n[sweep in={n_in} align={align}] largest error / limit {worst:.4f}")


# ------------------------------------------------------------------------------------------------ label kernels
def run_maskclip(dev, d, H, W, scale, th, ign):
    from semivl_amd import lib as L
    from semivl_amd import ops
    B, N, h, w = d.shape
    dd = d.to(dev)
    ig = None if ign is None else ign.to(dev)
    buf, out = guarded((B, H, W), dev, torch.int64)
    L.check(L.load().svl_maskclip_labels(ops._p(dd), B, N, h, w, H, W, float(scale), float(th), ops._p(ig), ops._p(out), ops._st()))
    torch.cuda.synchronize()
    assert guards_intact(buf)
    return out.cpu()


@pytest.mark.parametrize("name", [c[0] for c in R.maskclip_cases()])
def test_maskclip_labels(dev, name):
    _, d, H, W, th, ign = next(c for c in R.maskclip_cases() if c[0] == name)
    lab, cgap, gap, zb, cb = R.maskclip_labels(d, H, W, 100.0, th, ign)
    got = run_maskclip(dev, d, H, W, 100.0, th, ign)
    ok = torch.ones_like(lab, dtype=torch.bool) if name in ("N1", "const_tie") else (gap > 2 * zb) & (cgap > cb)
    assert 1.0 - ok.double().mean().item() <= 0.01
    print(f"\n[svl_maskclip_labels {name}] labels compared {ok.double().mean().item():.4f}, 255 on {(lab == 255).double().mean().item():.3f}")
    assert torch.equal(got[ok], lab[ok])
    if ign is not None:
        assert bool((got[ign == 255] == 255).all())


def test_maskclip_labels_beyond_one_pass(dev):
    g = torch.Generator().manual_seed(9)
    d = torch.randn(1, 2, 8, 8, generator=g) * 0.05
    assert 1025 * 1025 > ONE_PASS
    lab, cgap, gap, zb, cb = R.maskclip_labels(d, 1025, 1025, 100.0, 0.9, None)
    got = run_maskclip(dev, d, 1025, 1025, 100.0, 0.9, None)
    ok = (gap > 2 * zb) & (cgap > cb)
    assert 1.0 - ok.double().mean().item() <= 0.01
    assert torch.equal(got[ok], lab[ok]) and 0.05 < (lab == 255).double().mean().item() < 0.95


@pytest.mark.parametrize("HW,why", [(4 * ONE_PASS + 8, "float4 path: two quads beyond the capped grid"),
                                    (ONE_PASS + 3, "scalar path (odd HW): three pixels beyond it")])
def test_softmax_max_beyond_one_pass(dev, HW, why):
    g = torch.Generator().manual_seed(10)
    x = torch.randn(1, 2, HW, generator=g) * 2
    conf, lab, _ = R.softmax_max(x)
    gc, gl = run_softmax_max(dev, x.to(dev))
    r = R.ratio((gc.double().cpu() - conf).abs(), R.conf_bound(x))
    note("svl_softmax_max_f32 conf", r)
    assert r <= 1.0 and torch.equal(gl.cpu(), lab)


CONCEPT_CASES = [(2, [0, 1, 2, 3], 37), (2, [0, 2, 3, 7], 35), (1, [0, 5], 1), (1, [0, 1, 3], 2 * ONE_PASS + 5)]


@pytest.mark.parametrize("B,off,HW", CONCEPT_CASES)
def test_concept_max_is_bit_equal(dev, B, off, HW):
    """Groups of one class, mixed groups, one group, odd HW; the last case is just beyond four elements per thread of the
    capped grid (N HW = 4 x 4096 x 256 + 10)."""
    from semivl_amd import lib as L
    from semivl_amd import ops
    N, NC = len(off) - 1, off[-1]
    g = torch.Generator().manual_seed(11)
    pred = torch.randn(B, NC, HW, generator=g)
    buf, out = guarded((B, N, HW), dev)
    pd, od = pred.to(dev), torch.tensor(off, dtype=torch.int32, device=dev)
    L.check(L.load().svl_concept_max_f32(ops._p(pd), B, NC, HW, ops._p(od), N, ops._p(out), ops._st()))
    torch.cuda.synchronize()
    assert guards_intact(buf) and torch.equal(out.cpu(), R.concept_max(pred, off, N))


def _box(B, HW, g):
    """0 / 1 boxes with a few values that are not exactly 1.0 (0.999, 2.0, the fp32 next to 1) -- they select `a`."""
    box = (torch.rand(B, HW, generator=g) < 0.4).float()
    flat = box.view(-1)
    for k, v in enumerate((0.999, 2.0, float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0))))):
        flat[k::11][:max(1, flat.numel() // 40)] = v
    return box


@pytest.mark.parametrize("B,Cc,HW", [(2, 1, 37), (2, 3, 35), (1, 3, 1), (1, 3, (4 * ONE_PASS) // 3 + 7)])
def test_cutmix_f32_is_bit_equal(dev, B, Cc, HW):
    """C = 1 and 3, odd HW, box values other than exactly 1.0; the last case is just beyond four elements per thread."""
    from semivl_amd import lib as L
    from semivl_amd import ops
    g = torch.Generator().manual_seed(12)
    a, b, box = torch.randn(B, Cc, HW, generator=g), torch.randn(B, Cc, HW, generator=g), _box(B, HW, g)
    buf, out = guarded((B, Cc, HW), dev)
    ad, bd, xd = a.to(dev), b.to(dev), box.to(dev)
    L.check(L.load().svl_cutmix_f32(ops._p(out), ops._p(ad), ops._p(bd), ops._p(xd), B, Cc, HW, ops._st()))
    torch.cuda.synchronize()
    assert guards_intact(buf) and torch.equal(out.cpu(), R.cutmix(a, b, box))


@pytest.mark.parametrize("B,HW", [(2, 37), (3, 1), (1, 4 * ONE_PASS + 9)])
def test_cutmix_i64_is_bit_equal(dev, B, HW):
    from semivl_amd import lib as L
    from semivl_amd import ops
    g = torch.Generator().manual_seed(13)
    a, b, box = torch.randint(0, 256, (B, HW), generator=g), torch.randint(0, 256, (B, HW), generator=g), _box(B, HW, g)
    a[a == SENTINEL], b[b == SENTINEL] = 0, 0
    buf, out = guarded((B, HW), dev, torch.int64)
    ad, bd, xd = a.to(dev), b.to(dev), box.to(dev)
    L.check(L.load().svl_cutmix_i64(ops._p(out), ops._p(ad), ops._p(bd), ops._p(xd), B, HW, ops._st()))
    torch.cuda.synchronize()
    assert guards_intact(buf) and torch.equal(out.cpu(), R.cutmix(a, b, box))


@pytest.mark.parametrize("n", [1, 37, 2049, 8 * ONE_PASS + 13])
def test_count_valid_is_exact(dev, n):
    """The last size is just beyond eight elements per thread of the capped grid; the count adds to what the slot holds."""
    from semivl_amd import ops
    g = torch.Generator().manual_seed(14)
    m = torch.randint(0, 21, (n,), generator=g)
    m[torch.rand(n, generator=g) < 0.3] = 255
    m[::7] = 254
    buf = torch.full((3,), SENTINEL, dtype=torch.int64, device=dev)
    buf[1] = 5
    ops.count_valid(m.to(dev), buf[1:2])
    torch.cuda.synchronize()
    assert buf.tolist() == [SENTINEL, 5 + R.count_valid(m), SENTINEL]


def test_zz_largest_error_over_limit_per_kernel():
    """Not a check of its own: prints the largest error / limit the tests above have seen, per kernel and figure."""
    print()
    for k in sorted(WORST):
        print(f"largest error / limit, {k}: {WORST[k]:.4f}")
        assert WORST[k] <= 1.0
    assert math.isfinite(sum(WORST.values()))
