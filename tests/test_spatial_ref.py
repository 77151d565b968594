"""CPU: the restatements of tests/spatial_ref.py proved against independent expressions (fp32 F.interpolate of one-hot rows
for the 1-D bilinear weights; float64 F.interpolate / F.avg_pool2d / F.adaptive_avg_pool2d / F.conv2d / F.max_pool2d and
their autograd for the rest), and the derived bounds measured on the very inputs tests/test_spatial_kernels_gpu.py uses: a
plain fp32 torch evaluation on the CPU has to stay inside each of them.  -s prints the measured-to-bound ratios."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spatial_ref as S

TIGHT = 1e-12
SIZES = [(7, 20), (13, 45), (12, 51), (5, 33), (33, 9), (17, 40), (1, 11), (6, 1), (128, 512), (204, 801), (100, 400), (5, 17)]


def _close(a, b, tol=TIGHT):
    scale = max(1.0, float(b.abs().max()))
    return float((a - b).abs().max()) <= tol * scale


def _ratio(got, want, bound):
    """max |got - want| / bound over the elements with a positive bound; elements with a zero bound must be equal."""
    err = (got.double() - want).abs()
    z = bound <= 0
    assert bool((err[z] == 0).all())
    return float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ bilinear: the 1-D weights
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_axis_weights_are_the_weights_torch_uses(size, align):
    """fp32 F.interpolate of the one-hot rows of an identity IS the weight matrix torch uses.  It forms the coordinate in fp32
    from the same fp32 scale, so its weights agree with the float64 ones within axis_slack (the coordinate term) plus the
    one rounding of 1 - lambda."""
    inp, out = size
    eye = torch.eye(inp).view(inp, 1, 1, inp)
    Wt = F.interpolate(eye, size=(1, out), mode="bilinear", align_corners=align)[:, 0, 0, :].t().double()
    Wm, dW = S.axis_weights(inp, out, align), S.axis_slack(inp, out, align)
    assert Wm.shape == (out, inp) and _close(Wm.sum(1), torch.ones(out, dtype=torch.float64))
    assert bool(((Wt - Wm).abs() <= dW + 2 * S.U).all()), float(((Wt - Wm).abs() - dW).max())
    for shift in (-1, 1):       # the slack covers the shifted weights themselves
        assert bool(((S.axis_weights(inp, out, align, shift) - Wm).abs() <= dW * (1 + 1e-9) + 1e-18).all())


def test_axis_weights_landmarks():
    """Values that follow from the definition alone: align_corners maps the corners onto the corners; a single output pixel
    reads source 0 (scale 0); x2 without align_corners has the 0.25 / 0.75 pattern and a clamped first pixel."""
    Wm = S.axis_weights(5, 17, True)
    assert Wm[0, 0] == 1 and Wm[16, 4] == 1 and Wm[4, 1] == 1 and Wm[2, 0] == 0.5 and Wm[2, 1] == 0.5
    assert torch.equal(S.axis_weights(6, 1, True), torch.tensor([[1.0, 0, 0, 0, 0, 0]], dtype=torch.float64))
    W2 = S.axis_weights(4, 8, False)
    assert W2[0, 0] == 1 and W2[1, 0] == 0.75 and W2[1, 1] == 0.25 and W2[2, 0] == 0.25 and W2[2, 1] == 0.75 and W2[7, 3] == 1
    assert S.area_scale(7, 20, False) == float(np.float32(7) / np.float32(20)) != 7 / 20


# ------------------------------------------------------------------------------------------------ bilinear: the 2-D forms
def _interp64(x, H, W, align, rep):
    y = F.interpolate(_nchw(x.double()), size=(H, W), mode="bilinear", align_corners=align)
    return _nhwc(y).repeat_interleave(rep, 0)


@pytest.mark.parametrize("case", S.NHWC_CASES, ids=lambda c: c[0])
def test_bilinear_refs_vs_float64_interpolate_and_autograd(case):
    """Forward = float64 F.interpolate, backward = its autograd (with the repeat and the accumulation).  Torch's float64 scale
    is in / out in double, the restatement's is the fp32 quotient: the coordinates differ by less than s 2^-24 <= delta, so
    the allowance is the coordinate term alone (and 1e-12 where the fp32 quotient is exact)."""
    name, imgs, (h, w), (H, W), C, align, rep = case
    x, dy, by, bx = S.nhwc_inputs(case)
    xr = x.double().requires_grad_()
    want = _interp64(xr, H, W, align, rep)
    y, _, coord = S.bilinear_fwd_ref(x, H, W, align, rep, parts=True)
    assert y.shape == (imgs * rep, H, W, C)
    assert bool(((y - want.detach()).abs() <= coord + TIGHT).all())
    ya, _ = S.bilinear_fwd_ref(x, H, W, align, rep, base=by)
    assert _close(ya, y + by.double())
    want.backward(dy.double())
    dx, _, dcoord = S.bilinear_bwd_ref(dy, h, w, align, rep, parts=True)
    assert dx.shape == (imgs, h, w, C)
    assert bool(((dx - xr.grad).abs() <= dcoord + TIGHT).all())
    dxa, _ = S.bilinear_bwd_ref(dy, h, w, align, rep, base=bx)
    assert _close(dxa, dx + bx.double())
    exact = all(S.area_scale(a, b, align) == ((a - 1) / (b - 1) if align and b > 1 else 0.0 if align else a / b)
                for a, b in ((h, H), (w, W)))
    if exact:
        assert _close(y, want.detach()) and _close(dx, xr.grad)


def test_bilinear_bwd_is_the_transpose_of_the_forward():
    """<y, dy> == <x, dx> in float64, non-square, both conventions, up and down."""
    for case in S.NHWC_CASES:
        name, imgs, (h, w), (H, W), C, align, rep = case
        x, dy, _, _ = S.nhwc_inputs(case)
        y, _ = S.bilinear_fwd_ref(x, H, W, align, rep)
        dx, _ = S.bilinear_bwd_ref(dy, h, w, align, rep)
        a, b = float((y * dy.double()).sum()), float((x.double() * dx).sum())
        assert abs(a - b) <= 1e-10 * max(1.0, abs(a)), name


@pytest.mark.parametrize("case", S.NHWC_CASES + [S.NHWC_BIG_FWD, S.NHWC_BIG_BWD], ids=lambda c: c[0])
def test_fp32_interpolate_stays_inside_the_bilinear_bounds(case):
    """torch's own fp32 F.interpolate (forward, accumulated forward, autograd backward with the repeat) on the GPU file's
    inputs: inside the derived bound."""
    name, imgs, (h, w), (H, W), C, align, rep = case
    x, dy, by, bx = S.nhwc_inputs(case)
    xr = x.clone().requires_grad_()
    y32 = _nhwc(F.interpolate(_nchw(xr), size=(H, W), mode="bilinear", align_corners=align)).repeat_interleave(rep, 0)
    y, b = S.bilinear_fwd_ref(x, H, W, align, rep)
    r1 = _ratio(y32.detach(), y, b)
    ya, ba = S.bilinear_fwd_ref(x, H, W, align, rep, base=by)
    r2 = _ratio(by + y32.detach(), ya, ba)
    y32.backward(dy)
    dx, db = S.bilinear_bwd_ref(dy, h, w, align, rep)
    r3 = _ratio(xr.grad, dx, db)
    print(f"[cpu fp32 bilinear {name}] error / bound: fwd {r1:.3f}, fwd accumulate {r2:.3f}, bwd {r3:.3f}")
    assert max(r1, r2, r3) <= 1.0, (name, r1, r2, r3)


@pytest.mark.parametrize("case", S.PLANES_CASES + [S.PLANES_BIG_FWD, S.PLANES_BIG_BWD], ids=lambda c: c[0])
def test_fp32_interpolate_stays_inside_the_planes_bounds(case):
    name, planes, (h, w), (H, W), align = case
    x, dy = S.planes_inputs(case)
    xr = x.clone().requires_grad_()
    y32 = F.interpolate(xr[None], size=(H, W), mode="bilinear", align_corners=align)[0]
    y, b = S.bilinear_fwd_ref(x[..., None], H, W, align)
    r1 = _ratio(y32.detach()[..., None], y, b)
    y32.backward(dy)
    dx, db = S.bilinear_bwd_ref(dy[..., None], h, w, align)
    r2 = _ratio(xr.grad[..., None], dx, db)
    want = F.interpolate(x.double()[None], size=(H, W), mode="bilinear", align_corners=align)[0]
    assert float((y[..., 0] - want).abs().max()) <= float(b.max()) + TIGHT
    print(f"[cpu fp32 planes {name}] error / bound: fwd {r1:.3f}, bwd {r2:.3f}")
    assert max(r1, r2) <= 1.0, (name, r1, r2)


# ------------------------------------------------------------------------------------------------ sum_rep
@pytest.mark.parametrize("case", S.SUM_REP_CASES, ids=str)
def test_sum_rep_ref(case):
    rep, groups, rows, C, ld, off = case
    src = S._rand((groups * rep, rows, C), 10 + rep)
    out, b = S.sum_rep_ref(src, rep)
    want = torch.stack([sum(src[g * rep + r].double() for r in range(rep)) for g in range(groups)])
    assert out.shape == (groups, rows, C) and _close(out, want)
    acc = torch.zeros(groups, rows, C)
    for r in range(rep):                                      # a plain fp32 chain
        acc = acc + src.view(groups, rep, rows, C)[:, r]
    if rep <= 2:
        assert torch.equal(acc, out.float())
    else:
        assert _ratio(acc, out, b) <= 1.0


# ------------------------------------------------------------------------------------------------ average pool + concat
@pytest.mark.parametrize("case", S.POOL_CASES + [S.POOL_BIG], ids=lambda c: c[0])
def test_avgpool_cat_refs_vs_torch(case):
    """Forward = F.avg_pool2d (floor mode) / F.adaptive_avg_pool2d for the global form, concatenated with text[img % nclass];
    backward and text gradient = float64 autograd of that expression; fp32 torch inside the bounds."""
    name, imgs, (H, W), C, (PH, PW), Ct, nclass = case
    x, text, dy, base = S.pool_inputs(case)
    Hp, Wp = H // PH, W // PW

    def expr(xv, tv):
        p = F.avg_pool2d(_nchw(xv), (PH, PW))
        if (PH, PW) == (H, W) and xv.dtype == torch.float64:
            assert _close(p.detach(), F.adaptive_avg_pool2d(_nchw(xv), 1).detach())
        p = _nhwc(p)
        if tv is None:
            return p
        t = torch.stack([tv[i % nclass] for i in range(imgs)])[:, None, None, :].expand(imgs, Hp, Wp, Ct)
        return torch.cat((p, t), 3)

    xr = x.double().requires_grad_()
    tr = text.double().requires_grad_() if Ct else None
    want = expr(xr, tr)
    y, b = S.avgpool_cat_fwd_ref(x, PH, PW, text, nclass)
    assert y.shape == (imgs, Hp, Wp, C + Ct) and _close(y, want.detach())
    if Ct:
        assert torch.equal(y[..., C:].float(), expr(x, text)[..., C:]) and float(b[..., C:].abs().max()) == 0.0
    want.backward(dy.double())
    dx, db = S.avgpool_cat_bwd_ref(dy, H, W, C, PH, PW)
    assert _close(dx, xr.grad)
    assert float(dx[:, Hp * PH:].abs().sum()) == 0.0 and float(dx[:, :, Wp * PW:].abs().sum()) == 0.0
    dxa, dba = S.avgpool_cat_bwd_ref(dy, H, W, C, PH, PW, base=base)
    assert _close(dxa, dx + base.double())
    assert torch.equal(dxa[:, Hp * PH:].float(), base[:, Hp * PH:]) and float(dba[:, Hp * PH:].max() if Hp * PH < H else 0.0) <= \
        S.U * float(base.abs().max())
    # fp32 torch inside the bounds
    x32 = x.clone().requires_grad_()
    t32 = text.clone().requires_grad_() if Ct else None
    y32 = expr(x32, t32)
    y32.backward(dy)
    r = [_ratio(y32.detach(), y, b), _ratio(x32.grad, dx, db), _ratio(base + x32.grad, dxa, dba)]
    if Ct:
        dt, dtb = S.avgpool_text_bwd_ref(dy, C, nclass)
        assert dt.shape == (nclass, Ct) and _close(dt, tr.grad)
        r.append(_ratio(t32.grad, dt, dtb))
    print(f"[cpu fp32 avgpool {name}] error / bound: " + ", ".join(f"{v:.3f}" for v in r))
    assert max(r) <= 1.0, (name, r)


# ------------------------------------------------------------------------------------------------ thin convolutions
def _conv_same(xn, wt, KH, KW, dil, pad):
    """F.conv2d with the padding that makes off(tap) = (ti dil - pad, tj dil - pad) and the output H x W."""
    return F.conv2d(F.pad(xn, (pad, dil * (KW - 1) - pad, pad, dil * (KH - 1) - pad)), wt, dilation=dil)


@pytest.mark.parametrize("case", S.COUT1_CASES + S.WGRAD_EXTRA + [S.COUT1_BIG], ids=lambda c: c[0])
def test_conv_cout1_refs_vs_conv2d(case):
    name, imgs, (H, W), C, (KH, KW), dil, pad, gn, ld, off = case
    x, wf, bias, gn_in, dy = S.cout1_inputs(case)
    xop = S.gn_operand(x, gn_in) if gn else x.double()
    if gn:
        g = gn_in.double()
        exact = x.double() * g[:, 0][:, None, None, :] + g[:, 1][:, None, None, :]
        assert bool(((xop > 0) == (exact.float() > 0)).all())
        assert torch.equal(xop.float().double(), xop)
        assert bool(((xop - exact.clamp_min(0)).abs() <= S.U * exact.abs()).all())
    wt = wf.double().view(1, KH, KW, C).permute(0, 3, 1, 2).contiguous().requires_grad_()      # forward pack -> OIHW
    xn = _nchw(xop)
    want = _conv_same(xn, wt, KH, KW, dil, pad)[:, 0] + bias.double()
    y, b = S.conv_cout1_fwd_ref(xop, wf, bias, KH, KW, dil, pad, gn)
    assert y.shape == (imgs, H, W) and _close(y, want.detach())
    y32 = _conv_same(_nchw(xop.float()), wt.detach().float(), KH, KW, dil, pad)[:, 0] + bias
    r = [_ratio(y32, y, b)]
    if (KH, KW) == (3, 3):
        want.backward(dy.double())
        dw, dwb = S.conv_cout1_wgrad_ref(dy, xop, dil, pad)
        assert dw.shape == (9 * C,) and _close(dw, wt.grad.permute(0, 2, 3, 1).reshape(-1))
        w32 = wt.detach().float().requires_grad_()
        (_conv_same(_nchw(xop.float()), w32, 3, 3, dil, pad)[:, 0] * dy).sum().backward()
        r.append(_ratio(w32.grad.permute(0, 2, 3, 1).reshape(-1), dw, dwb))
    print(f"[cpu fp32 conv_cout1 {name}] error / bound: " + ", ".join(f"{v:.3f}" for v in r))
    assert max(r) <= 1.0, (name, r)


@pytest.mark.parametrize("case", S.TAP_CASES + [S.TAP_BIG], ids=lambda c: c[0])
def test_tap_gather_ref_vs_conv2d(case):
    """sign = +1: the input gradient of Conv2d(1 -> Co) in its split T = dY . Wtap^T, then the gather (autograd of F.conv2d);
    sign = -1: the forward of Conv2d(1 -> 1) with T[p][tap] = x[p] w[tap]."""
    name, imgs, (H, W), (KH, KW), dil, pad, sign = case
    big = H * W > 100000
    T = S.tap_inputs(case)
    out, b = S.tap_gather_ref(T, KH, KW, dil, pad, sign)
    acc = torch.zeros(imgs, H, W)
    for t, (dh, dw) in enumerate(S.tap_offsets(KH, KW, dil, pad)):       # a plain fp32 chain over the taps
        acc = acc + S.shifted(T[..., t], -sign * dh, -sign * dw)
    assert _ratio(acc, out, b) <= 1.0
    Co = 1 if big else 5
    g = torch.Generator().manual_seed(77)
    wt = torch.randn(Co, 1, KH, KW, generator=g, dtype=torch.float64)
    if sign == 1:
        x = torch.zeros(imgs, 1, H, W, dtype=torch.float64, requires_grad=True)
        dY = torch.randn(imgs, Co, H, W, generator=g, dtype=torch.float64)
        _conv_same(x, wt, KH, KW, dil, pad).backward(dY)
        Tm = torch.einsum("nohw,ot->nhwt", dY, wt.view(Co, KH * KW))
        got, _ = S.tap_gather_ref(Tm, KH, KW, dil, pad, 1)
        assert _close(got, x.grad[:, 0])
    else:
        x = torch.randn(imgs, 1, H, W, generator=g, dtype=torch.float64)
        Tm = x[:, 0, :, :, None] * wt[0].reshape(-1)
        got, _ = S.tap_gather_ref(Tm, KH, KW, dil, pad, -1)
        assert _close(got, _conv_same(x, wt[:1], KH, KW, dil, pad)[:, 0])


# ------------------------------------------------------------------------------------------------ max pool
@pytest.mark.parametrize("case", S.MAXPOOL_CASES, ids=lambda c: c[0])
def test_maxpool_ref_vs_max_pool2d(case):
    """Values and winners = F.max_pool2d(3, 2, 1, return_indices=True) with its flat indices mapped to tap numbers; backward =
    float64 autograd."""
    name, imgs, (H, W), C, ties = case
    x, dy = S.maxpool_inputs(case)
    y, idx = S.maxpool_ref(x)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xr = _nchw(x.double()).requires_grad_()
    want, flat = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    assert y.shape == (imgs, Ho, Wo, C) and torch.equal(y.double(), _nhwc(want.detach()))
    ih, iw = flat // W, flat % W
    oh = torch.arange(Ho)[None, None, :, None]
    ow = torch.arange(Wo)[None, None, None, :]
    taps = (ih - (2 * oh - 1)) * 3 + (iw - (2 * ow - 1))
    assert torch.equal(idx.long(), _nhwc(taps))
    if ties:
        assert bool((idx[0, :, :, 0] == torch.where(torch.arange(Ho) == 0, 3, 0)[:, None] +
                     torch.where(torch.arange(Wo) == 0, 1, 0)[None, :]).all())     # constant plane: first tap inside the image
    want.backward(_nchw(dy.double()))
    dx, b = S.maxpool_bwd_ref(dy, idx, H, W)
    assert _close(dx, _nhwc(xr.grad))
    x32 = _nchw(x).requires_grad_()
    F.max_pool2d(x32, 3, 2, 1).backward(_nchw(dy))
    assert _ratio(_nhwc(x32.grad), dx, b) <= 1.0
