"""GPU: the kernels of csrc/maskclip_refine.hip (svl_mc_softmax_f32, svl_mc_class_peak_f32, svl_col_invsq_f32, svl_mc_select_f32)
and ops.mc_refine around the two svl_gemm_f32 products, held to the float64 restatement tests/maskclip_refine_ref.py (which is
held to the reference's own code by tests/test_maskclip_refine_ref.py).

Inputs come from maskclip_refine_ref.draw_case: every peak and every row maximum of the float64 restatement is at least 1e-3 from
its threshold, so DECISIONS are compared for equality: the dropped-class set, the smoothed-row set.  The kernels' `peak` and
`rowmax` are fp32 maxima of the kernel's own fp32 P: they are held bit for bit to the maxima of that P (a maximum rounds nothing)
and, through P's bound, to the restatement's values.  Values are held to bounds derived from the number formats alone
(maskclip_refine_ref's docstring): P, s, the product stage from the kernel's own P and s (mode 0: gamma(HW + E + 4) times the sum
of the addends' magnitudes), and end to end from raw inputs (that, plus sum_j |W_ij| times P's bound).  In arithmetic mode 6 a
product that the library routes to an fp32 kernel family keeps the fp32 bound; one that runs on a split-product family gets the
gate the svl_gemm_f32 descriptor tests apply to those families (tests/test_gemm_desc_gpu.py): norm-wise error against float64
<= 1.2 x the error of the same launch in mode 0.

Layouts: contiguous and 16-byte aligned (the float4 forms) and padded leading dimensions with every pointer 4 bytes off a
16-byte boundary (the scalar forms); sentinel guard bands and padding columns must come back intact; a second run gives the same
bits.  `-s` prints the worst error / bound ratios."""
import ctypes as C
import functools

import pytest
import torch

import maskclip_refine_ref as R
from spatial_ref import AGUARD, SENTINEL, gaps_intact, strided

pytestmark = pytest.mark.gpu

PD, KS = 0.5, 0.7
SHAPES = [(1, 1, 1, 64), (1, 2, 2, 64), (2, 63, 5, 64), (2, 64, 21, 128), (3, 65, 21, 64), (1, 768, 150, 768), (2, 1024, 21, 768),
          (2, 96, 24, 68)]      # the last: N % 4 == 0 (the float4 form of the class peak), E % 32 != 0, a ragged second token tile
LAYOUTS = ("aligned", "odd")
EMU6_ERR_FACTOR = 1.2          # tests/test_gemm_desc_gpu.py: the gate of every split-product kernel family
FP32_PATHS = (0, 2, 3)
WORST = {}


def _ids(s):
    return "x".join(str(v) for v in s)


@pytest.fixture
def emu_mode():
    from semivl_amd import ops
    yield ops.set_gemm_emulation
    ops.set_gemm_emulation(0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"worst error / bound, {k}: {WORST[k]:.3f}")


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def _ratio(err, bound):
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    return float(r.nan_to_num(nan=float("inf")).max())


@functools.lru_cache(None)
def case(shape, nan=False):
    """(x, k fp32 on the host, the float64 restatement, P64 / its bound, s64 / its bound), computed once per shape."""
    B, HW, N, E = shape
    x, k = R.draw_case(B, HW, N, E, 1000 + sum(shape), PD, KS, nan_at=(0, min(3, HW - 1), min(1, N - 1)) if nan else None)
    r = R.refine_ref(x, k, PD, KS)
    assert min(R.margins(r, PD, KS)) >= R.MARGIN
    P64, pb = R.p_bound(x, r["dropped"])
    s64, sb = R.s_ref(k.reshape(B * HW, E), B, HW)
    return x, k, r, P64, pb, s64, sb


def _lib():
    from semivl_amd import lib as L_
    return L_, L_.load()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _mat(t2d, layout, dev):
    """(buffer, view, ld, off): the matrix on the device, contiguous and aligned, or padded and 4 bytes off."""
    rows, Cc = t2d.shape
    ld, off = (Cc, 0) if layout == "aligned" else (Cc + 7, 1)
    buf, v = strided(rows, Cc, ld, off, dev)
    if t2d.dtype == torch.float32:
        v.copy_(t2d)
    return buf, v, ld, off


def _vec(n, layout, dev):
    """(buffer, view) of n floats; "odd": 4 bytes off a 16-byte boundary."""
    off = 0 if layout == "aligned" else 1
    buf = torch.full((n + 2 * AGUARD + off,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[AGUARD + off:AGUARD + off + n]


def _vec_intact(buf, n, layout):
    off = 0 if layout == "aligned" else 1
    return bool((buf[:AGUARD + off] == SENTINEL).all()) and bool((buf[AGUARD + off + n:] == SENTINEL).all())


def _stages(shape, layout, dev, nan=False):
    """The four passes launched through the C ABI on guarded buffers; returns what they wrote (device tensors) + intactness."""
    L_, lib = _lib()
    B, HW, N, E = shape
    x, k = case(shape, nan)[:2]
    rows = B * HW
    xb, xv, ldx, xo = _mat(x.reshape(rows, N), layout, dev)
    kb, kv, ldk, ko = _mat(k.reshape(rows, E), layout, dev)
    p0b, p0v, ldp, po = _mat(torch.empty(rows, N, dtype=torch.float64), layout, dev)
    pb_, pv, _, _ = _mat(torch.empty(rows, N, dtype=torch.float64), layout, dev)
    peakb, peak = _vec(B * N, layout, dev)
    rmb, rowmax = _vec(rows, layout, dev)
    sbuf, s = _vec(B * E, layout, dev)
    chk = lambda rc, what: L_.check(rc, what)
    chk(lib.svl_mc_softmax_f32(_p(xv), ldx, None, 0.0, B, HW, N, 0, _p(p0v), ldp, None, _st()), "softmax 0")
    chk(lib.svl_mc_class_peak_f32(_p(p0v), ldp, B, HW, N, _p(peak), _st()), "peak")
    chk(lib.svl_mc_softmax_f32(_p(xv), ldx, _p(peak), PD, B, HW, N, 0, _p(pv), ldp, _p(rowmax), _st()), "softmax")
    chk(lib.svl_col_invsq_f32(_p(kv), ldk, B, HW, E, 1e-12, _p(s), _st()), "invsq")
    torch.cuda.synchronize()
    intact = (gaps_intact(xb, rows, N, ldx, xo) and gaps_intact(kb, rows, E, ldk, ko) and gaps_intact(p0b, rows, N, ldp, po)
              and gaps_intact(pb_, rows, N, ldp, po) and _vec_intact(peakb, B * N, layout) and _vec_intact(rmb, rows, layout)
              and _vec_intact(sbuf, B * E, layout))
    return dict(x=xv, k=kv, P0=p0v, P=pv, peak=peak.view(B, N), rowmax=rowmax, s=s.view(B, E), intact=intact)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_stage_kernels(dev, shape, layout):
    B, HW, N, E = shape
    x, k, r, P64, pb, s64, sb = case(shape)
    g = _stages(shape, layout, dev)
    assert g["intact"], "a guard band or a padding column was written"
    P0, P, peak, rowmax, s = (g[n].cpu() for n in ("P0", "P", "peak", "rowmax", "s"))
    # maxima: exact functions of the kernel's own fp32 P
    assert torch.equal(_bits(peak), _bits(P0.view(B, HW, N).max(1).values))
    assert torch.equal(_bits(rowmax), _bits(P.max(1).values))
    # decisions: the restatement's
    assert torch.equal(peak < PD, r["dropped"]) and torch.equal(rowmax < KS, r["selected"].reshape(-1))
    # values
    P0_64, p0b = R.p_bound(x, torch.zeros_like(r["dropped"]))
    e0, e1, es = (P0.double() - P0_64).abs(), (P.double() - P64).abs(), (s.double() - s64).abs()
    ratios = (_ratio(e0, p0b), _ratio(e1, pb), _ratio(es, sb))
    print(f"{_ids(shape)} {layout}: error / bound  P0 {ratios[0]:.3f}  P {ratios[1]:.3f}  s {ratios[2]:.3f}")
    for name, v in zip(("P0", "P", "s"), ratios):
        _note(name, v)
    assert max(ratios) <= 1.0, ratios
    # the peak against the restatement's, through P0's bound (a maximum moves at most as far as its operands)
    assert bool(((peak.double() - r["peak"]).abs() <= p0b.view(B, HW, N).max(1).values).all())
    assert bool(((rowmax.double() - r["rowmax"].reshape(-1)).abs() <= pb.max(1).values).all())
    g2 = _stages(shape, layout, dev)
    for n in ("P0", "P", "peak", "rowmax", "s"):
        assert torch.equal(_bits(g2[n].cpu()), _bits(g[n].cpu())), f"{n}: a second run gave other bits"


def _normwise(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_product_stage_and_end_to_end(dev, emu_mode, monkeypatch, shape):
    """The two products from the kernel's own fp32 P and s, then ops.mc_refine from raw inputs, in modes 0 and 6."""
    from semivl_amd import ops
    _, lib = _lib()
    B, HW, N, E = shape
    x, k, r, P64, pb, s64, sb = case(shape)
    xd, kd = x.reshape(B * HW, N).to(dev), k.reshape(B * HW, E).to(dev)
    paths = []
    real_gemm = ops.gemm

    def gemm(*a, **kw):
        real_gemm(*a, **kw)
        paths.append(lib.svl_last_gemm_path())

    monkeypatch.setattr(ops, "gemm", gemm)
    base = {}
    for mode in (0, 6):
        emu_mode(mode)
        del paths[:]
        out, parts = ops.mc_refine(xd, kd, B, HW, PD, KS, return_parts=True)
        torch.cuda.synchronize()
        e2e_paths = tuple(paths)
        P32, s32 = parts["P"].cpu(), parts["s"].cpu()
        assert torch.equal(parts["selected"].cpu(), r["selected"].reshape(-1))
        assert torch.equal(parts["peak"].cpu() < PD, r["dropped"])
        assert _ratio((P32.double() - P64).abs(), pb) <= 1.0 and _ratio((s32.double() - s64).abs(), sb) <= 1.0
        # ---- the product stage alone, on the kernel's own P and s
        del paths[:]
        O = ops.mc_smooth(parts["P"], kd, parts["s"], B, HW).cpu()
        torch.cuda.synchronize()
        assert tuple(paths) == e2e_paths and len(paths) == 2
        O64, ob = R.product_ref(P32, k.reshape(B * HW, E), s32, B, HW)
        # ---- end to end: selected rows against the restatement from raw inputs
        sel = r["selected"].reshape(-1)
        got = out.cpu().transpose(1, 2).reshape(B * HW, N)
        W = k.double() @ (s32.double().view(B, -1, 1) * k.double().transpose(1, 2))        # k diag(s) k^T in float64
        e2e_bound = ob + (W.abs() @ pb.view(B, HW, N)).reshape(B * HW, N)
        want = r["out"].transpose(1, 2).reshape(B * HW, N)
        assert torch.equal(_bits(got[~sel]), _bits(P32[~sel])), "an unsmoothed row is not P's bits"
        assert torch.equal(_bits(got[sel]), _bits(O[sel])), "a smoothed row is not the product stage's bits"
        fp32 = all(p in FP32_PATHS for p in paths)
        if fp32:
            rs, re = _ratio((O.double() - O64).abs(), ob), (_ratio((got.double() - want).abs()[sel], e2e_bound[sel]) if sel.any() else 0.0)
            print(f"{_ids(shape)} mode {mode} paths {paths}: error / bound  product stage {rs:.3f}  end to end {re:.3f}")
            _note(f"product stage, mode {mode}", rs)
            _note(f"end to end, mode {mode}", re)
            assert rs <= 1.0 and re <= 1.0, (mode, rs, re)
        else:
            ns = _normwise(O.double(), O64)
            ne = _normwise(got.double()[sel], want[sel]) if sel.any() else 0.0
            print(f"{_ids(shape)} mode {mode} paths {paths}: norm-wise  product stage {ns:.3e} (mode 0 {base['ns']:.3e})  "
                  f"end to end {ne:.3e} (mode 0 {base['ne']:.3e})")
            assert ns <= EMU6_ERR_FACTOR * base["ns"] and ne <= EMU6_ERR_FACTOR * base["ne"], (ns, ne, base)
        if mode == 0:
            assert fp32, "mode 0 runs the fp32 kernels"
            base = dict(ns=_normwise(O.double(), O64), ne=_normwise(got.double()[sel], want[sel]) if sel.any() else 0.0)
        out2 = ops.mc_refine(xd, kd, B, HW, PD, KS)
        assert torch.equal(_bits(out2.cpu()), _bits(out.cpu())), "a second run gave other bits"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_select_writes_planes_and_nothing_else(dev, shape, layout):
    L_, lib = _lib()
    B, HW, N, E = shape
    g = torch.Generator().manual_seed(5)
    rows = B * HW
    P, O = torch.randn(rows, N, generator=g), torch.randn(rows, N, generator=g)
    rowmax = torch.rand(rows, generator=g)
    rowmax[::7] = float("nan")
    _, Pv, ldp, _ = _mat(P, layout, dev)
    _, Ov, ldo, _ = _mat(O, layout, dev)
    rb, rv = _vec(rows, layout, dev)
    rv.copy_(rowmax)
    ob, ov = _vec(B * N * HW, layout, dev)
    L_.check(lib.svl_mc_select_f32(_p(Pv), ldp, _p(Ov), ldo, _p(rv), KS, B, HW, N, _p(ov), _st()), "select")
    torch.cuda.synchronize()
    want = torch.where((rowmax < KS)[:, None], O, P).view(B, HW, N).transpose(1, 2).contiguous()
    assert torch.equal(_bits(ov.cpu().view(B, N, HW)), _bits(want)) and _vec_intact(ob, B * N * HW, layout)
    ob2, ov2 = _vec(B * N * HW, layout, dev)
    L_.check(lib.svl_mc_select_f32(_p(Pv), ldp, None, 0, None, 0.0, B, HW, N, _p(ov2), _st()), "select")
    torch.cuda.synchronize()
    assert torch.equal(_bits(ov2.cpu().view(B, N, HW)), _bits(P.view(B, HW, N).transpose(1, 2).contiguous()))
    assert _vec_intact(ob2, B * N * HW, layout)


def test_nan_logit_gives_the_restatements_nan_set(dev):
    from semivl_amd import ops
    shape = (2, 63, 5, 64)
    B, HW, N, E = shape
    x, k, r = case(shape, True)[:3]
    out, parts = ops.mc_refine(x.reshape(B * HW, N).to(dev), k.reshape(B * HW, E).to(dev), B, HW, PD, KS, return_parts=True)
    assert torch.equal(torch.isnan(out.cpu()), torch.isnan(r["out"]))
    assert torch.equal(torch.isnan(parts["peak"].cpu()), torch.isnan(r["peak"]))
    assert torch.equal(torch.isnan(parts["rowmax"].cpu()), torch.isnan(r["rowmax"].reshape(-1)))
    assert torch.equal(parts["peak"].cpu() < PD, r["dropped"]) and torch.equal(parts["selected"].cpu(), r["selected"].reshape(-1))
    assert bool(torch.isnan(r["out"][0]).any()) and not bool(torch.isnan(r["out"][1]).any())
    g = _stages(shape, "odd", dev, nan=True)
    assert g["intact"] and torch.equal(torch.isnan(g["peak"].cpu()), torch.isnan(r["peak"]))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_thresholds_off_and_prompt_denoising_alone(dev, shape):
    from semivl_amd import ops
    B, HW, N, E = shape
    x, k, r = case(shape)[:3]
    xd, kd = x.reshape(B * HW, N).to(dev), k.reshape(B * HW, E).to(dev)
    planes = x.transpose(1, 2).contiguous()
    for keys in (None, kd):
        out, parts = ops.mc_refine(xd, keys, B, HW, 0.0, 0.0, return_parts=True)
        assert torch.equal(_bits(out.cpu()), _bits(planes)) and parts["P"] is xd and parts["selected"] is None
    assert torch.equal(_bits(ops.mc_refine(xd, None, B, HW, 0.0, KS).cpu()), _bits(planes))      # no keys: nothing to smooth with
    out = ops.mc_refine(xd, kd, B, HW, PD, 0.0).cpu()
    dropped = r["dropped"][:, :, None].expand(B, N, HW)
    assert bool((out[dropped] == -100.0).all()) and torch.equal(_bits(out[~dropped]), _bits(planes[~dropped]))
    buf = torch.full((B, N, HW), SENTINEL, device=dev)
    assert ops.mc_refine(xd, kd, B, HW, PD, KS, out=buf) is buf and not bool((buf == SENTINEL).any())


def test_wrappers_match_the_entry_points(dev):
    from semivl_amd import ops
    shape = (3, 65, 21, 64)
    B, HW, N, E = shape
    g = _stages(shape, "aligned", dev)
    xd, kd = g["x"].contiguous(), g["k"].contiguous()
    P0, _ = ops.mc_softmax(xd, B, HW, want_rowmax=False)
    assert torch.equal(_bits(ops.mc_class_peak(P0, B, HW)), _bits(g["peak"].contiguous()))
    assert torch.equal(_bits(ops.col_invsq(kd, B, HW)), _bits(g["s"].contiguous()))
    P, rowmax = ops.mc_softmax(xd, B, HW, g["peak"].contiguous(), PD)
    assert torch.equal(_bits(P), _bits(g["P"].contiguous())) and torch.equal(_bits(rowmax), _bits(g["rowmax"].contiguous()))
    for bad in (-1.0, True, "0.5", float("nan")):
        with pytest.raises(ValueError, match="pd_thresh"):
            ops.mc_refine(xd, kd, B, HW, bad, KS)
        with pytest.raises(ValueError, match="ks_thresh"):
            ops.mc_refine(xd, kd, B, HW, PD, bad)


def test_refusals_by_name(dev):
    L_, lib = _lib()
    t = torch.zeros(64, device=dev)
    p, st = _p(t), _st()

    def refused(rc, *words):
        msg = L_.last_error()
        assert rc == -1 and all(w in msg for w in words), (rc, msg, words)

    refused(lib.svl_mc_class_peak_f32(None, 4, 1, 4, 4, p, st), "svl_mc_class_peak_f32", "null pointer")
    refused(lib.svl_mc_class_peak_f32(p, 4, 1, 4, 4, None, st), "svl_mc_class_peak_f32", "null pointer")
    refused(lib.svl_mc_class_peak_f32(p, 4, 0, 4, 4, p, st), "svl_mc_class_peak_f32", "B 0")
    refused(lib.svl_mc_class_peak_f32(p, 4, 1, 0, 4, p, st), "svl_mc_class_peak_f32", "HW 0")
    refused(lib.svl_mc_class_peak_f32(p, 4, 1, 4, 0, p, st), "svl_mc_class_peak_f32", "N 0")
    refused(lib.svl_mc_class_peak_f32(p, 3, 1, 4, 4, p, st), "svl_mc_class_peak_f32", "ld 3 below the width N 4")
    refused(lib.svl_col_invsq_f32(None, 4, 1, 4, 4, 1e-12, p, st), "svl_col_invsq_f32", "null pointer")
    refused(lib.svl_col_invsq_f32(p, 4, 1, 4, 4, 1e-12, None, st), "svl_col_invsq_f32", "null pointer")
    refused(lib.svl_col_invsq_f32(p, 4, -1, 4, 4, 1e-12, p, st), "svl_col_invsq_f32", "B -1")
    refused(lib.svl_col_invsq_f32(p, 4, 1, 0, 4, 1e-12, p, st), "svl_col_invsq_f32", "HW 0")
    refused(lib.svl_col_invsq_f32(p, 4, 1, 4, 0, 1e-12, p, st), "svl_col_invsq_f32", "E 0")
    refused(lib.svl_col_invsq_f32(p, 3, 1, 4, 4, 1e-12, p, st), "svl_col_invsq_f32", "ld 3 below the width E 4")
    refused(lib.svl_col_invsq_f32(p, 4, 1, 4, 4, -1.0, p, st), "svl_col_invsq_f32", "eps")
    refused(lib.svl_mc_softmax_f32(None, 4, None, 0.0, 1, 4, 4, 0, p, 4, None, st), "svl_mc_softmax_f32", "null pointer")
    refused(lib.svl_mc_softmax_f32(p, 4, None, 0.0, 1, 4, 4, 0, None, 4, None, st), "svl_mc_softmax_f32", "null pointer")
    refused(lib.svl_mc_softmax_f32(p, 4, None, 0.0, 0, 4, 4, 0, p, 4, None, st), "svl_mc_softmax_f32", "B 0")
    refused(lib.svl_mc_softmax_f32(p, 4, None, 0.0, 1, 0, 4, 0, p, 4, None, st), "svl_mc_softmax_f32", "HW 0")
    refused(lib.svl_mc_softmax_f32(p, 4, None, 0.0, 1, 4, 0, 0, p, 4, None, st), "svl_mc_softmax_f32", "N 0")
    refused(lib.svl_mc_softmax_f32(p, 3, None, 0.0, 1, 4, 4, 0, p, 4, None, st), "svl_mc_softmax_f32", "ldx 3", "below the width")
    refused(lib.svl_mc_softmax_f32(p, 4, None, 0.0, 1, 4, 4, 0, p, 3, None, st), "svl_mc_softmax_f32", "ldp 3", "below the width")
    refused(lib.svl_mc_softmax_f32(p, 4, None, -0.5, 1, 4, 4, 0, p, 4, None, st), "svl_mc_softmax_f32", "pd_thresh")
    refused(lib.svl_mc_softmax_f32(p, 4, None, 0.0, 1, 4, 4, 1, p, 4, p, st), "svl_mc_softmax_f32", "fill_only")
    refused(lib.svl_mc_select_f32(None, 4, None, 0, None, 0.0, 1, 4, 4, p, st), "svl_mc_select_f32", "null pointer")
    refused(lib.svl_mc_select_f32(p, 4, None, 0, None, 0.0, 1, 4, 4, None, st), "svl_mc_select_f32", "null pointer")
    refused(lib.svl_mc_select_f32(p, 4, p, 4, None, 0.0, 1, 4, 4, p, st), "svl_mc_select_f32", "O and rowmax")
    refused(lib.svl_mc_select_f32(p, 4, None, 0, None, 0.0, 0, 4, 4, p, st), "svl_mc_select_f32", "B 0")
    refused(lib.svl_mc_select_f32(p, 4, None, 0, None, 0.0, 1, 0, 4, p, st), "svl_mc_select_f32", "HW 0")
    refused(lib.svl_mc_select_f32(p, 4, None, 0, None, 0.0, 1, 4, 0, p, st), "svl_mc_select_f32", "N 0")
    refused(lib.svl_mc_select_f32(p, 3, None, 0, None, 0.0, 1, 4, 4, p, st), "svl_mc_select_f32", "ldp 3", "below the width")
    refused(lib.svl_mc_select_f32(p, 4, p, 3, p, 0.0, 1, 4, 4, p, st), "svl_mc_select_f32", "ldo 3", "below the width")
    refused(lib.svl_mc_select_f32(p, 4, p, 4, p, -1.0, 1, 4, 4, p, st), "svl_mc_select_f32", "ks_thresh")
    torch.cuda.synchronize()
    assert bool((t == 0).all()), "a refused call wrote"
