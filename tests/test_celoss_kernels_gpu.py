"""GPU: the label-smoothing / class-weight variants of the two cross-entropy kernels (svl_ce_fused_lsw_f32,
svl_ce_up_fused_lsw_f32) and the two normaliser kernels (svl_class_weight_sum_f64, svl_scale_from_sum_f32) against the
float64 restatement of tests/celoss_ref.py (which tests/test_celoss_ref.py holds to torch's float64 loss and autograd).

Limits (celoss_ref.LOSS_TOL / D_RTOL / GRAD_*): those tests/test_pixel_loss_up_gpu.py holds the plain kernel to, with the
absolute part of the gradient limit restated relative to the gradient scale g (there g = 1 / nval ~ 5e-4, atol 2e-8 = 4e-5 g).
torch's own fp32 loss lies inside them on the same inputs (tests/test_celoss_ref.py).  Error / limit is printed (-s).

Zero sum over the classes: every pixel's gradient is a p_c - b [c = t] - e w_c with a = b + e W, so it sums to a (sum_c p_c - 1)
plus rounding.  p_c = e_c / s with s the fp32 sum of N exponentials (relative error <= N u, u = 2^-24), and each of the N
elements carries a few roundings of terms whose magnitudes add up to a + b + e W = 2 a: |sum_c d_c| <= (N + 8) u 2 a.  A
head-resolution cell gathers its pixels with the resize's non-negative weights, which do not depend on the class: the same
bound carried through the resize's transpose, plus one rounding per gathered term (<= 2 u sum |d|)."""
import functools

import numpy as np
import pytest
import torch

import celoss_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64                 # floats (doubles for the sums) of NaN on either side of every output
U = 2.0 ** -24


def guarded(shape, dev, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()) and \
        not bool(torch.isnan(buf[GUARD:-GUARD]).any())


@functools.lru_cache(None)
def fused_case(B, N, HW, name):
    eps, w = R.setting(name, N)
    x, t = R.logits_and_target((B, N, HW), (B, HW), N, seed=11)
    g = float(np.float32(1.0 / R.celoss(x, t, eps, w)["D"].item()))      # the scale the kernel reads, as the fp32 it is
    return x, t, eps, w, g, R.celoss(x, t, eps, w, g=g)


@functools.lru_cache(None)
def up_case(N, h, w_, H, W, align, name):
    eps, w = R.setting(name, N)
    x, t = R.logits_and_target((2, N, h, w_), (2, H, W), N, seed=12)
    g = float(np.float32(1.0 / R.celoss_up(x, H, W, align, t, eps, w)["D"].item()))
    return x, t, eps, w, g, R.celoss_up(x, H, W, align, t, eps, w, g=g)


def pixel_sum_bound(t, eps, w, g, N):
    """(N + 8) u 2 a per pixel (module docstring), float64 [B, *]; 0 on ignored pixels."""
    wv = torch.ones(N, dtype=torch.float64) if w is None else w.double()
    v = t != 255
    wt = torch.where(v, wv[torch.where(v, t, torch.zeros_like(t))], torch.zeros((), dtype=torch.float64))
    a = g * ((1.0 - eps) * wt + (eps / N) * wv.sum()) * v
    return (N + 8) * U * 2.0 * a


def check_against(ref, sums, dl, t, w, g, what):
    loss = (sums[0] / sums[3]).item()
    e_loss = abs(loss - ref["loss"].item())
    D = ref["D"].item()
    e_D = abs(sums[3].item() - D) / D
    err = (dl.double().cpu() - ref["grad"]).abs()
    ratio = (err / (R.GRAD_ATOL_G * g + R.GRAD_RTOL * ref["grad"].abs())).max().item()
    print(f"\n[{what}] loss |d| {e_loss:.2e} / {R.LOSS_TOL:.0e}; D rel {e_D:.2e} / {R.D_RTOL:.0e}; gradient error / limit {ratio:.4f}")
    assert e_loss < R.LOSS_TOL, (loss, ref["loss"].item())
    assert e_D <= R.D_RTOL
    if w is None:
        assert sums[3].item() == float((t != 255).sum().item())
    assert sums[1].item() == 0.0 and sums[2].item() == 0.0
    assert torch.allclose(dl.double().cpu(), ref["grad"], atol=R.GRAD_ATOL_G * g, rtol=R.GRAD_RTOL), ratio
    return ratio


# ------------------------------------------------------------------------------------------------ ce_fused
@pytest.mark.parametrize("name", R.SETTINGS)
@pytest.mark.parametrize("B,N,HW", R.FUSED_SHAPES)
def test_ce_fused_lsw(dev, B, N, HW, name):
    from semivl_amd import ops
    x, t, eps, w, g, ref = fused_case(B, N, HW, name)
    xd, td = x.to(dev), t.to(dev)
    wd = None if w is None else w.to(dev)
    gs = torch.tensor([g, 0.0], device=dev)
    dbuf, dl = guarded((B, N, HW), dev)
    sbuf, sums = guarded((4,), dev, torch.float64)
    ops.ce_fused(xd, td, True, dlogits=dl, gscale=gs, sums_out=sums, label_smoothing=eps, class_weight=wd)
    torch.cuda.synchronize()
    assert guards_intact(dbuf) and guards_intact(sbuf)
    check_against(ref, sums.cpu(), dl, t, w, g, f"ce_fused B{B} N{N} HW{HW} {name}")
    # every pixel's gradient sums to zero over the classes; ignored pixels are exactly 0
    rows = dl.double().cpu().movedim(1, -1)
    assert bool((rows.sum(-1).abs() <= pixel_sum_bound(t, eps, w, g, N) + 1e-300).all())
    assert bool((rows[t == 255] == 0).all())
    # two runs, bit for bit; the forward-only call gives the same sums
    dl2 = torch.full_like(dl, float("nan"))
    s2 = ops.ce_fused(xd, td, True, dlogits=dl2, gscale=gs, label_smoothing=eps, class_weight=wd)
    s3 = ops.ce_fused(xd, td, True, label_smoothing=eps, class_weight=wd)
    assert torch.equal(dl2, dl) and torch.equal(s2, sums) and torch.equal(s3, sums)
    # every target ignored: D = 0, the scale is 1 / 0 and multiplies nothing
    dbuf0, dl0 = guarded((B, N, HW), dev)
    s0 = ops.ce_fused(xd, torch.full_like(td, 255), True, dlogits=dl0, gscale=torch.tensor([float("inf"), 0.0], device=dev),
                      label_smoothing=eps, class_weight=wd)
    assert guards_intact(dbuf0) and bool((dl0 == 0).all()) and s0.tolist() == [0.0, 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ ce_up_fused
@pytest.mark.parametrize("name", R.SETTINGS)
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("N,h,w_,H,W", R.UP_GEOMS)
def test_ce_up_fused_lsw(dev, N, h, w_, H, W, align, name):
    from semivl_amd import ops
    B = 2
    x, t, eps, w, g, ref = up_case(N, h, w_, H, W, align, name)
    xd, td = x.to(dev), t.to(dev)
    wd = None if w is None else w.to(dev)
    gs = torch.tensor([g, 0.0], device=dev)
    kw = dict(label_smoothing=eps, class_weight=wd)

    def run(target, scale):
        dbuf, dl = guarded((B, N, h, w_), dev)
        sbuf, sums = guarded((4,), dev, torch.float64)
        if fused:
            ops.ce_up_fused(xd, H, W, align, target, True, dlogits=dl, gscale=scale, sums_out=sums, **kw)
        else:       # the caller's fallback: resize, the full-resolution kernel, the resize's backward
            full = ops.bilinear_planes_fwd(xd, h, w_, align, H, W)
            dfull = torch.full_like(full, float("nan"))
            ops.ce_fused(full, target, True, dlogits=dfull, gscale=scale, sums_out=sums, **kw)
            dl.copy_(ops.bilinear_planes_bwd(dfull, h, w_, align, H, W))
        torch.cuda.synchronize()
        assert guards_intact(dbuf) and guards_intact(sbuf)
        return dl, sums

    fused = ops.ce_up_lsw_ok(B, N, h, w_, H, W, align)
    if not fused:   # the refusal is real, and the resized path agrees instead
        with pytest.raises(RuntimeError, match="unsupported geometry"):
            ops.ce_up_fused(xd, H, W, align, td, True, gscale=gs, **kw)
    dl, sums = run(td, gs)
    check_against(ref, sums.cpu(), dl, t, w, g, f"ce_up_fused N{N} {h}x{w_}->{H}x{W} align={align} {name} fused={fused}")
    # every head-resolution cell's gradient sums to zero over the classes
    bound = R.resize_transpose(pixel_sum_bound(t, eps, w, g, N).unsqueeze(1), h, w_, align)[:, 0]
    bound = bound + 2 * U * dl.double().abs().sum(1).cpu()
    assert bool((dl.double().sum(1).cpu().abs() <= bound + 1e-300).all())
    dl2, s2 = run(td, gs)
    assert torch.equal(dl2, dl) and torch.equal(s2, sums)
    dl0, s0 = run(torch.full_like(td, 255), torch.tensor([float("inf"), 0.0], device=dev))
    assert bool((dl0 == 0).all()) and s0.tolist() == [0.0, 0.0, 0.0, 0.0]


def test_ignored_band_leaves_its_cells_exactly_zero(dev):
    """Rows 4..11 of image 0 are ignored: at ratio 2 the head-resolution rows 3 and 4 have their whole footprint (rows 5..8,
    7..10) inside the band and get exactly 0 in every class (no pixel of theirs is multiplied by anything)."""
    from semivl_amd import ops
    N, h, w_, H, W = 4, 17, 11, 34, 22
    x, t, eps, w, g, ref = up_case(N, h, w_, H, W, False, "eps0.2_zero_weight")
    assert ops.ce_up_lsw_ok(2, N, h, w_, H, W, False)
    dl = torch.full((2, N, h, w_), float("nan"), device=dev)
    ops.ce_up_fused(x.to(dev), H, W, False, t.to(dev), True, dlogits=dl, gscale=torch.tensor([g, 0.0], device=dev),
                    label_smoothing=eps, class_weight=w.to(dev))
    dead = (ref["grad_full"][0].abs().sum(0) == 0).all(1)        # full-resolution rows without any gradient
    assert dead[4:12].all()
    cells = R.resize_matrix(h, H, False)[~dead].sum(0) == 0      # head rows touched by dead rows only
    assert cells.nonzero().flatten().tolist() == [3, 4]
    assert bool((dl[0][:, cells.to(dev)] == 0).all())


# ------------------------------------------------------------------------------------------------ the plain path stays
def test_zero_smoothing_and_no_weight_is_the_plain_entry_point(dev):
    from semivl_amd import ops
    x, t, *_ = fused_case(2, 21, 672, "eps0.1")
    xd, td = x.to(dev), t.to(dev)
    gs = torch.tensor([1e-3, 0.0], device=dev)
    a, b = torch.empty_like(xd), torch.empty_like(xd)
    sa = ops.ce_fused(xd, td, True, dlogits=a, gscale=gs)
    sb = ops.ce_fused(xd, td, True, dlogits=b, gscale=gs, label_smoothing=0.0, class_weight=None)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    x, t, *_ = up_case(5, 8, 8, 32, 32, False, "eps0.1")
    xd, td = x.to(dev), t.to(dev)
    a, b = torch.empty_like(xd), torch.empty_like(xd)
    sa = ops.ce_up_fused(xd, 32, 32, False, td, True, dlogits=a, gscale=gs)
    sb = ops.ce_up_fused(xd, 32, 32, False, td, True, dlogits=b, gscale=gs, label_smoothing=0.0, class_weight=None)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    # all-ones weights and no smoothing through the variant: the plain loss, to rounding
    c = torch.empty_like(xd)
    sc = ops.ce_up_fused(xd, 32, 32, False, td, True, dlogits=c, gscale=gs, class_weight=torch.ones(5, device=dev))
    assert sc[3].item() == sa[3].item() and abs((sc[0] / sc[3]).item() - (sa[0] / sa[3]).item()) < 1e-6
    assert torch.allclose(c, a, atol=4e-5 * 1e-3, rtol=2e-4)


def test_unlabelled_descriptors_are_refused_by_name(dev):
    from semivl_amd import lib as L
    from semivl_amd import ops
    x, t, *_ = fused_case(2, 21, 672, "eps0.1")
    xd, td = x.to(dev), t.to(dev)
    conf = torch.rand(2, 672, device=dev)
    ign = torch.zeros(2, 672, dtype=torch.int64, device=dev)
    for kw, field in ((dict(conf=conf, ign=ign), "conf"), (dict(mc=td), "mc_target"), (dict(img_weight=conf[:, 0].contiguous()), "img_weight"),
                      (dict(all_pixels=True), "all_pixels")):
        with pytest.raises(RuntimeError, match=field):
            ops.ce_fused(xd, td, True, label_smoothing=0.1, **kw)
        assert field in L.last_error() and "svl_ce_fused_lsw_f32" in L.last_error()
    with pytest.raises(RuntimeError, match="use_ignore_t"):
        ops.ce_fused(xd, td, False, label_smoothing=0.1)
    x, t, *_ = up_case(5, 8, 8, 32, 32, False, "eps0.1")
    xd, td = x.to(dev), t.to(dev)
    conf = torch.rand(2, 32, 32, device=dev)
    ign = torch.zeros(2, 32, 32, dtype=torch.int64, device=dev)
    for kw, field in ((dict(conf=conf, ign=ign), "conf"), (dict(mc=td), "mc_target")):
        with pytest.raises(RuntimeError, match=field):
            ops.ce_up_fused(xd, 32, 32, False, td, True, label_smoothing=0.1, **kw)
        assert field in L.last_error() and "svl_ce_up_fused_lsw_f32" in L.last_error()
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.ce_fused(xd.view(2, 5, 64), td.view(2, 1024)[:, :64].contiguous(), True, label_smoothing=1.5)
    with pytest.raises(ValueError, match="class_weight"):
        ops.ce_fused(xd.view(2, 5, 64), td.view(2, 1024)[:, :64].contiguous(), True, class_weight=torch.ones(4, device=dev))


# ------------------------------------------------------------------------------------------------ the normaliser
def test_class_weight_sum_is_the_exact_double(dev):
    """fp32 weights in [0.5, 1.5] are multiples of 2^-24 below 2: a sum of fewer than 2^28 of them is exact in double in any
    order, so the kernel's fixed-order sum equals the histogram's sum bit for bit."""
    from semivl_amd import ops
    N = 21
    g = torch.Generator().manual_seed(3)
    t = torch.randint(0, N, (3, 211, 97), generator=g)           # 61401 pixels: no multiple of the chunks or the block
    t[torch.rand(3, 211, 97, generator=g) < 0.1] = 255
    w = (torch.rand(N, generator=g) + 0.5).float()
    want = (torch.bincount(t[t != 255].flatten(), minlength=N).double() * w.double()).sum().item()
    buf, out = guarded((1,), dev, torch.float64)
    ops.class_weight_sum(t.to(dev), w.to(dev), out)
    torch.cuda.synchronize()
    assert guards_intact(buf) and out.item() == want
    out2 = torch.empty(1, dtype=torch.float64, device=dev)
    assert ops.class_weight_sum(t.to(dev), w.to(dev), out2).item() == want
    assert ops.class_weight_sum(torch.full((5, 7), 255, dtype=torch.int64, device=dev), w.to(dev), out2).item() == 0.0
    t1 = torch.tensor([[3]], dtype=torch.int64, device=dev)      # a single pixel: most chunks are empty
    assert ops.class_weight_sum(t1, w.to(dev), out2).item() == float(w[3])


@pytest.mark.parametrize("s,factor", [(3.0, 1.0), (12345.678, 0.5), (2.0 ** 31 + 1.5, 1.0), (0.7, 0.5)])
def test_scale_from_sum_is_the_correctly_rounded_float(dev, s, factor):
    from semivl_amd import ops
    out = torch.full((2,), -7.0, device=dev)
    ops.scale_from_sum(torch.tensor([s], dtype=torch.float64, device=dev), factor, out)
    torch.cuda.synchronize()
    assert np.float32(out[0].item()) == np.float32(np.float64(factor) / np.float64(s))
    assert out[1].item() == -7.0
