"""Plain float64 / int64 restatements of the memory-bound spatial kernels of the VLG head and the conv encoder --
svl_bilinear_nhwc_fwd / _bwd, svl_bilinear_planes_fwd / _bwd, svl_sum_rep_f32, svl_avgpool_cat_fwd / _bwd / _bwd_text,
svl_conv_cout1_fwd / _wgrad (with gn_in), svl_tap_gather, svl_maxpool3x3s2_fwd / _bwd -- each from the header's formula
(include/semivl_hip.h) or the ATen definition it names (upsample_bilinear2d: area_pixel_compute_source_index +
guard_index_and_lambda; max_pool2d: first maximum in scan order), none from the kernels.  Device-agnostic, like
tests/small_kernel_ref.py, whose guard-band helpers and unit roundoff it reuses: tests/test_spatial_kernels_gpu.py runs them on
the device with ATen as the checker, tests/test_spatial_ref.py proves them on the CPU against independent expressions.

Also here: the DERIVED error bounds (each with its derivation) and the seeded case builders both test files share, so the CPU
file can show that a plain fp32 evaluation stays inside the bounds on the very inputs the GPU file uses.

Bounds: a chain of n fp32 operations (sums and products, fused or not) on terms t_k errs by at most gamma(n) * sum |t_k|,
gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1 / section 3.1)."""
import numpy as np
import torch

from small_kernel_ref import GUARD, SENTINEL, U, guard_intact, guarded  # noqa: F401  (re-exported for the two test files)

RESAMPLE_GRID_CAP = 256 * 32     # blocks of 256 threads `grid_for` (csrc/resample.hip) and `grid1d` (csrc/batchnorm.hip) launch at most
THIN_GRID_CAP = 256 * 16         # the same for svl_conv_cout1_fwd (generic form) and svl_tap_gather (csrc/conv_thin.hip)
AGUARD = 64                      # guard elements that keep a payload 16-byte aligned (R.GUARD = 61 does not: the scalar paths)


def gamma(n):
    return n * U / (1.0 - n * U)


def one_pass(cap=RESAMPLE_GRID_CAP, per_block=256):
    """Work items one pass of a capped grid covers."""
    return cap * per_block


def strided(rows, C, ld, off, device, fill=SENTINEL, guard=AGUARD):
    """(buffer, [rows, C] view): rows `ld` apart starting at column `off` of a [rows, ld] matrix of `fill`, `guard` more
    elements of `fill` on each side.  off % 4 == 0 and ld % 4 == 0 keep every row 16-byte aligned."""
    assert off + C <= ld
    buf = torch.full((rows * ld + 2 * guard,), fill, dtype=torch.float32, device=device)
    return buf, buf[guard:guard + rows * ld].view(rows, ld)[:, off:off + C]


def gaps_intact(buf, rows, C, ld, off, fill=SENTINEL, guard=AGUARD):
    """The guard bands and the columns [0, off) and [off + C, ld) of every row still hold `fill`."""
    m = buf[guard:guard + rows * ld].view(rows, ld)
    ok = bool((buf[:guard] == fill).all()) and bool((buf[guard + rows * ld:] == fill).all())
    return ok and bool((m[:, :off] == fill).all()) and bool((m[:, off + C:] == fill).all())


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ bilinear resize
def area_scale(inp, out, align):
    """ATen's area_pixel_compute_scale<float>: ONE fp32 division; align_corners with a single output pixel gives 0."""
    if align:
        return float(np.float32(inp - 1) / np.float32(out - 1)) if out > 1 else 0.0
    return float(np.float32(inp) / np.float32(out))


def axis_coords(inp, out, align):
    """float64 source coordinate of every destination index, from the fp32 scale, BEFORE the clamp at 0."""
    sc = area_scale(inp, out, align)
    d = np.arange(out, dtype=np.float64)
    return sc * d if align else sc * (d + 0.5) - 0.5


def coord_delta(s):
    """delta = 2 ulp_fp32(max(|s|, 1)): the kernel (and ATen) form the coordinate in fp32 from the same fp32 scale as
    fl(fl(scale * (d + 0.5)) - 0.5) or one fused multiply-add.  d + 0.5 is exact; the product errs by half an ulp of s + 0.5
    (<= one ulp of max(|s|, 1): at most the next binade), the subtraction by half an ulp of s: 1.5 ulp <= delta."""
    return 2.0 * np.spacing(np.maximum(np.abs(s), 1.0).astype(np.float32)).astype(np.float64)


def axis_weights(inp, out, align, shift=0):
    """W [out, inp] float64, row d = the two tap weights of destination index d (guard_index_and_lambda): i0 = min(floor(s),
    inp - 1), i1 = min(i0 + 1, inp - 1), lambda = s - i0 clamped to [0, 1]; s is clamped at 0 (it is negative only for
    align_corners = False).  shift in {-1, 0, +1} moves every coordinate by shift * coord_delta first."""
    s = axis_coords(inp, out, align)
    s = np.maximum(s + shift * coord_delta(s), 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), inp - 1)
    i1 = np.minimum(i0 + 1, inp - 1)
    lam = np.clip(s - i0, 0.0, 1.0)
    Wm = np.zeros((out, inp), np.float64)
    r = np.arange(out)
    np.add.at(Wm, (r, i0), 1.0 - lam)
    np.add.at(Wm, (r, i1), lam)
    return torch.from_numpy(Wm)


def axis_slack(inp, out, align):
    """dW [out, inp] >= |W(s') - W(s)| entrywise for EVERY |s' - s| <= coord_delta(s): an entry of a row, as a function of
    the coordinate, is a hat function (with its clamped ends: constant 1 beyond either edge), hence 1-Lipschitz, and it is
    zero unless the coordinate lies within one of its source index.  So: delta on every source index a coordinate of
    [s - delta, s + delta] can touch, 0 elsewhere.  The interpolant is continuous across an integer crossing, so a different
    i0 inside that interval is covered by the same term."""
    s = axis_coords(inp, out, align)
    d = coord_delta(s)
    lo = np.clip(np.floor(np.maximum(s - d, 0.0)).astype(np.int64), 0, inp - 1)
    hi = np.clip(np.floor(np.maximum(s + d, 0.0)).astype(np.int64) + 1, 0, inp - 1)
    j = np.arange(inp)[None, :]
    return torch.from_numpy(((j >= lo[:, None]) & (j <= hi[:, None])) * d[:, None])


def _sep(Wy, x, Wx):
    """[n, Y, X, c] = Wy [Y, h] . x [n, h, w, c] . Wx [X, w]^T"""
    t = torch.einsum("Yh,nhwc->nYwc", Wy.to(x.device), x)
    return torch.einsum("Xw,nYwc->nYXc", Wx.to(x.device), t)


def _taps(Wm, dW):
    """Largest number of destination indices that can contribute to one source index."""
    return int(((Wm + dW) > 0).sum(0).max())


def bilinear_fwd_ref(x, H, W, align, rep=1, base=None, parts=False):
    """(y, bound), float64.  x [imgs, h, w, C] (a planes operand is C = 1) -> y [imgs * rep, H, W, C] = Wy . x . Wx^T, output
    image i from input image i / rep, plus `base` when accumulating.

    bound = gamma(6) * |Wy| |x| |Wx|^T + coordinate term (+ one rounding of the accumulating sum): the longest chain from an
    input to the output is 1 - lambda_x, lx * v, +, ly * (.), +, and 1 - lambda_y feeding the last product: 6 roundings.  The
    coordinate term is the change of the result when each axis' weights move by at most axis_slack (parts: returned third)."""
    x = x.double()
    h, w = x.shape[1], x.shape[2]
    Wy, Wx = axis_weights(h, H, align), axis_weights(w, W, align)
    dWy, dWx = axis_slack(h, H, align), axis_slack(w, W, align)
    y = _sep(Wy, x, Wx).repeat_interleave(rep, 0)
    mag = _sep(Wy, x.abs(), Wx)
    coord = _sep(Wy + dWy, x.abs(), Wx + dWx) - mag
    bound = (gamma(6) * mag + coord).repeat_interleave(rep, 0)
    if base is not None:
        y = y + base.double()
        bound = bound + U * (y.abs() + bound)
    return (y, bound, coord.repeat_interleave(rep, 0)) if parts else (y, bound)


def bilinear_bwd_ref(dy, h, w, align, rep=1, base=None, parts=False):
    """(dx, bound), float64.  dy [imgs * rep, H, W, C] -> dx [imgs, h, w, C] = sum over the rep images of Wy^T . dy . Wx (the
    transpose of the forward), plus `base` when accumulating.

    bound = gamma(n) * |Wy|^T sum_r |dy| |Wx| + coordinate term, n = max(T rep, T + rep) + 4: T = the largest number of
    (row, column) taps one input pixel collects; the kernel adds T * rep products in a chain, or (through svl_sum_rep_f32)
    rep terms first and T products then; each product carries 1 - lambda, wy * wx and wgt * d: 3 more, the accumulating sum 1."""
    H, W = dy.shape[1], dy.shape[2]
    d = dy.double().view(dy.shape[0] // rep, rep, H, W, dy.shape[3])
    Wy, Wx = axis_weights(h, H, align), axis_weights(w, W, align)
    dWy, dWx = axis_slack(h, H, align), axis_slack(w, W, align)
    dx = _sep(Wy.t(), d.sum(1), Wx.t())
    ad = d.abs().sum(1)
    mag = _sep(Wy.t(), ad, Wx.t())
    coord = _sep((Wy + dWy).t(), ad, (Wx + dWx).t()) - mag
    T = _taps(Wy, dWy) * _taps(Wx, dWx)
    bound = gamma(max(T * rep, T + rep) + 4) * mag + coord
    if base is not None:
        dx = dx + base.double()
        bound = bound + U * (dx.abs() + bound)
    return (dx, bound, coord) if parts else (dx, bound)


# ------------------------------------------------------------------------------------------------ sum_rep
def sum_rep_ref(src, rep):
    """(out, bound) float64: src [groups * rep, rows, C] -> out [groups, rows, C] = sum over r; bound = gamma(rep) sum |src|
    (a chain of at most rep additions); rep <= 2 is ONE correctly rounded addition (or none): out.float() is the answer."""
    s = src.double().view(src.shape[0] // rep, rep, *src.shape[1:])
    return s.sum(1), gamma(rep) * s.abs().sum(1)


# ------------------------------------------------------------------------------------------------ average pool + concat
def avgpool_cat_fwd_ref(x, PH, PW, text=None, nclass=1):
    """(y, bound) float64: x [imgs, H, W, C] -> y [imgs, H // PH, W // PW, C + Ct]; floor windows (rows / columns beyond
    Hp * PH / Wp * PW are not read); y[..., C:] = text[img % nclass] (exact: bound 0 there).
    bound = gamma(PH PW + 1) * mean |x|: PH PW - 1 additions, the rounded reciprocal 1 / (PH PW), one product."""
    x = x.double()
    imgs, H, W, C = x.shape
    Hp, Wp = H // PH, W // PW
    win = x[:, :Hp * PH, :Wp * PW].reshape(imgs, Hp, PH, Wp, PW, C)
    y = win.sum((2, 4)) / (PH * PW)
    b = gamma(PH * PW + 1) * win.abs().sum((2, 4)) / (PH * PW)
    if text is not None and text.shape[1] > 0:
        t = text.double()[torch.arange(imgs, device=x.device) % nclass]
        t = t[:, None, None, :].expand(imgs, Hp, Wp, text.shape[1])
        y, b = torch.cat((y, t), 3), torch.cat((b, torch.zeros_like(t)), 3)
    return y, b


def avgpool_cat_bwd_ref(dy, H, W, C, PH, PW, base=None):
    """(dx, bound) float64: dy [imgs, Hp, Wp, C + Ct] -> dx [imgs, H, W, C] = dy[img, y // PH, x // PW, :C] / (PH PW) inside
    the floor region, 0 outside (accumulate: `base` + that; outside the region base + 0 = base exactly).
    bound = gamma(2) |v| for the rounded reciprocal and the product, plus one rounding of the accumulating sum."""
    d = dy.double()[..., :C]
    imgs, Hp, Wp = d.shape[:3]
    v = torch.zeros(imgs, H, W, C, dtype=torch.float64, device=dy.device)
    v[:, :Hp * PH, :Wp * PW] = d.repeat_interleave(PH, 1).repeat_interleave(PW, 2) / (PH * PW)
    bound = gamma(2) * v.abs()
    if base is not None:
        v = v + base.double()
        bound = bound + U * (v.abs() + bound)
    return v, bound


def avgpool_text_bwd_ref(dy, C, nclass):
    """(dtext, bound) float64: dtext[n, ct] = sum over images with img % nclass == n and pooled pixels of dy[..., C + ct].
    bound = gamma(HWp + nb) sum |dy|: no addition order sums more than every pixel of an image and every image of a class."""
    d = dy.double()[..., C:]
    imgs, Ct = d.shape[0], d.shape[-1]
    HWp = d[0].numel() // Ct
    per = d.reshape(imgs, HWp, Ct)
    cls = torch.arange(imgs, device=dy.device) % nclass
    out = torch.zeros(nclass, Ct, dtype=torch.float64, device=dy.device).index_add_(0, cls, per.sum(1))
    mag = torch.zeros(nclass, Ct, dtype=torch.float64, device=dy.device).index_add_(0, cls, per.abs().sum(1))
    return out, gamma(HWp + imgs // nclass) * mag


# ------------------------------------------------------------------------------------------------ thin convolutions
def tap_offsets(KH, KW, dil, pad):
    """off(tap) = (ti * dil - pad, tj * dil - pad), tap = ti * KW + tj."""
    return [(ti * dil - pad, tj * dil - pad) for ti in range(KH) for tj in range(KW)]


def shifted(x, dh, dw):
    """z[n, i, j, ...] = x[n, i + dh, j + dw, ...] inside the image, 0 outside (x [n, H, W, ...])."""
    H, W = x.shape[1], x.shape[2]
    z = torch.zeros_like(x)
    i0, i1, j0, j1 = max(0, -dh), min(H, H - dh), max(0, -dw), min(W, W - dw)
    if i0 < i1 and j0 < j1:
        z[:, i0:i1, j0:j1] = x[:, i0 + dh:i1 + dh, j0 + dw:j1 + dw]
    return z


def gn_operand(x, gn_in):
    """relu(fma(x, scale, shift)) as fp32 values held in float64: x [imgs, H, W, C] fp32, gn_in [imgs, 2, C] fp32 (scale,
    shift).  The product of two fp32 numbers is exact in float64 and the float64 sum keeps the sign of the exact result, so
    the ReLU decision is the fused multiply-add's; rounding the float64 sum to fp32 is the fma's value except where the
    float64 sum sits within 2^-53 of an fp32 rounding boundary (then one ulp: the bounds count one operation for it)."""
    g = gn_in.double()
    v = x.double() * g[:, 0][:, None, None, :] + g[:, 1][:, None, None, :]
    return v.float().clamp_min(0.0).double()


def conv_cout1_fwd_ref(xop, wf, bias, KH, KW, dil, pad, gn=False):
    """(y, bound) float64: xop [imgs, H, W, C] (the operand: x, or gn_operand(x, gn_in)), wf [KH * KW * C] forward pack ->
    y [imgs, H, W] = bias + sum_{tap, c} xop[pix + off(tap)][c] * wf[tap * C + c], zero outside the image.
    bound = gamma(KH KW C + log2(C / 4) + 2) (sum |x| |w| + |bias|): one product and one addition per term fit the chain
    count of the sum, the shuffle tree across the C / 4 channel lanes adds log2(C / 4), the bias 1, the operand's fma 1."""
    x = xop.double()
    C = x.shape[3]
    wd = wf.double().reshape(KH * KW, C).to(x.device)
    y = torch.zeros(x.shape[:3], dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(y)
    for t, (dh, dw) in enumerate(tap_offsets(KH, KW, dil, pad)):
        s = shifted(x, dh, dw)
        y += s @ wd[t]
        mag += s.abs() @ wd[t].abs()
    b = 0.0 if bias is None else float(bias.double().reshape(-1)[0])
    n = KH * KW * C + max(int(np.log2(max(C // 4, 1))), 0) + 2 + (1 if gn else 0)
    return y + b, gamma(n) * (mag + abs(b))


def wgrad_chain(imgs, H, W, C):
    """Longest fp32 chain of svl_conv_cout1_wgrad + the slab sum: pixels per thread + PR + slabs (+ 2: the product, the
    operand's fma), with the launch geometry the header documents (svl_conv_cout1_wgrad_blocks blocks; a block's 256 threads
    are PR = 256 / (C / 4) pixel lanes)."""
    npix = imgs * H * W
    nb = min(2048, max(1, (npix + 4095) // 4096))
    PR = 256 // (C // 4)
    ppb = (npix + nb - 1) // nb
    return (ppb + PR - 1) // PR + PR + nb + 2, nb


def conv_cout1_wgrad_ref(dy, xop, dil, pad):
    """(dw, bound) float64: dy [imgs, H, W], xop [imgs, H, W, C] -> dw [9 * C] (forward pack) =
    sum_pix dy[pix] * xop[pix + off(tap)][c]; bound = gamma(wgrad_chain) * sum |dy| |xop|."""
    x, d = xop.double(), dy.double()
    imgs, H, W, C = x.shape
    out, mag = [], []
    for dh, dw in tap_offsets(3, 3, dil, pad):
        s = shifted(x, dh, dw)
        out.append(torch.einsum("nhw,nhwc->c", d, s))
        mag.append(torch.einsum("nhw,nhwc->c", d.abs(), s.abs()))
    n, _ = wgrad_chain(imgs, H, W, C)
    return torch.cat(out), gamma(n) * torch.cat(mag)


def tap_gather_ref(T, KH, KW, dil, pad, sign):
    """(out, bound) float64: T [imgs, H, W, KH * KW] -> out [imgs, H, W] = sum_tap T[p - sign * off(tap)][tap], zero outside
    the image; bound = gamma(KH KW) sum |T| (a chain of KH KW additions)."""
    Td = T.double()
    out = torch.zeros(Td.shape[:3], dtype=torch.float64, device=T.device)
    mag = torch.zeros_like(out)
    for t, (dh, dw) in enumerate(tap_offsets(KH, KW, dil, pad)):
        s = shifted(Td[..., t], -sign * dh, -sign * dw)
        out += s
        mag += s.abs()
    return out, gamma(KH * KW) * mag


# ------------------------------------------------------------------------------------------------ max pool 3x3, stride 2, pad 1
def maxpool_ref(x):
    """(y, idx): x [imgs, H, W, C] -> y [imgs, Ho, Wo, C] (same dtype, exact) and idx uint8 = the winning tap kh * 3 + kw of
    the window rows 2 oh - 1 + kh, columns 2 ow - 1 + kw, FIRST maximum in scan order; taps outside the image never win."""
    imgs, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    best = torch.full((imgs, Ho, Wo, C), -float("inf"), dtype=x.dtype, device=x.device)
    idx = torch.zeros((imgs, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    oh = torch.arange(Ho, device=x.device)
    ow = torch.arange(Wo, device=x.device)
    for k in range(9):
        ih, iw = 2 * oh - 1 + k // 3, 2 * ow - 1 + k % 3
        okh, okw = (ih >= 0) & (ih < H), (iw >= 0) & (iw < W)
        v = x[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)]
        ok = (okh[:, None] & okw[None, :])[None, :, :, None]
        win = ok & (v > best)
        best = torch.where(win, v, best)
        idx = torch.where(win, torch.full_like(idx, k), idx)
    return best, idx


def maxpool_bwd_ref(dy, idx, H, W):
    """(dx, bound) float64: every output element's gradient goes to the input element its idx names; an input element lies
    in at most 2 x 2 windows: bound = gamma(3) sum |dy|."""
    imgs, Ho, Wo, C = dy.shape
    k = idx.long()
    oh = torch.arange(Ho, device=dy.device)[None, :, None, None]
    ow = torch.arange(Wo, device=dy.device)[None, None, :, None]
    n = torch.arange(imgs, device=dy.device)[:, None, None, None]
    c = torch.arange(C, device=dy.device)[None, None, None, :]
    ih, iw = 2 * oh - 1 + k // 3, 2 * ow - 1 + k % 3
    assert bool(((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)).all())
    flat = (((n * H + ih) * W + iw) * C + c).reshape(-1)
    dx = torch.zeros(imgs * H * W * C, dtype=torch.float64, device=dy.device).index_add_(0, flat, dy.double().reshape(-1))
    mag = torch.zeros_like(dx).index_add_(0, flat, dy.double().abs().reshape(-1))
    return dx.view(imgs, H, W, C), gamma(3) * mag.view(imgs, H, W, C)


# ------------------------------------------------------------------------------------------------ shared cases
# Non-square in every pair of axes that could be exchanged.  (name, imgs, (h, w), (H, W), C, align, rep)
NHWC_CASES = [
    ("up_frac_ac0", 2, (7, 13), (20, 45), 8, False, 1),
    ("up_frac_ac1", 2, (7, 13), (20, 45), 8, True, 2),
    ("up_int_ac0", 3, (6, 11), (24, 33), 12, False, 3),          # x4 rows, x3 columns
    ("up_int_ac1", 1, (5, 9), (17, 25), 4, True, 5),             # (in - 1) | (out - 1): integer coordinates
    ("up_tall_ac0", 2, (12, 5), (51, 33), 16, False, 2),
    ("up_tall_ac1", 2, (12, 5), (51, 33), 16, True, 3),
    ("down_ac0", 2, (33, 17), (9, 40), 8, False, 3),
    ("down_ac1", 2, (33, 17), (9, 40), 8, True, 1),
    ("bcast_1x1_ac0", 3, (1, 1), (11, 23), 8, False, 2),
    ("bcast_1x1_ac1", 3, (1, 1), (11, 23), 8, True, 5),
    ("H1_ac1", 2, (6, 10), (1, 27), 8, True, 2),                 # scale 0 along y
    ("W1_ac1", 2, (6, 10), (19, 1), 8, True, 3),                 # scale 0 along x
    ("skip_form", 2, (32, 24), (64, 48), 32, False, 5),          # the head's skip resize (vlg_head.py:133), rep = classes
]
NHWC_BIG_FWD = ("fwd_two_passes", 2, (50, 57), (200, 231), 32, False, 3)      # 2 * 3 * 200 * 231 * 8 quads > 2^21
NHWC_BIG_BWD = ("bwd_two_passes", 4, (130, 131), (40, 37), 128, True, 2)      # 4 * 130 * 131 * 32 quads > 2^21


def nhwc_inputs(case):
    """(x [imgs, h, w, C], dy [imgs * rep, H, W, C], base_y like dy, base_x like x), fp32, seeded by the case's name."""
    name, imgs, (h, w), (H, W), C, align, rep = case
    seed = 5000 + sum(map(ord, name))
    return (_rand((imgs, h, w, C), seed), _rand((imgs * rep, H, W, C), seed + 1), _rand((imgs * rep, H, W, C), seed + 2),
            _rand((imgs, h, w, C), seed + 3))


# (name, planes, (h, w), (H, W), align)
PLANES_CASES = [
    ("step_128_512_ac0", 6, (32, 24), (128, 96), False),          # the step's x4 on a non-square map
    ("step_204_801_ac1", 2, (204, 153), (801, 601), True),        # the 801 crop's resize at its true fractional scale 203 / 800 (152 / 600 in x); W % 4 != 0: scalar forward
    ("quarter_ac1", 3, (51, 38), (201, 149), True),               # scales exactly 0.25: every coordinate a multiple of a quarter
    ("odd_W_ac0", 5, (9, 14), (30, 53), False),                   # W % 4 != 0
    ("fallback_x5_ac0", 4, (12, 7), (30, 36), False),             # ratio 5.14 in x only: more than 9 contributing columns
    ("fallback_x6_ac1", 4, (10, 6), (23, 41), True),              # ratio 8 in x (align), 2.4 in y
    ("down_ac0", 3, (33, 17), (9, 40), False),
    ("W1_ac1", 2, (6, 10), (19, 1), True),
    ("bcast_1x1", 3, (1, 1), (7, 12), False),
]
PLANES_BIG_FWD = ("fwd_two_passes", 42, (128, 100), (512, 400), False)        # 42 * 512 * 100 quads > 2^21
PLANES_BIG_BWD = ("bwd_two_passes", 130, (128, 130), (40, 36), False)         # 130 * 128 * 130 pixels > 2^21


def planes_inputs(case):
    name, planes, (h, w), (H, W), align = case
    seed = 6000 + sum(map(ord, name))
    return _rand((planes, h, w), seed), _rand((planes, H, W), seed + 1)


SUM_REP_CASES = [(rep, groups, rows, C, ld, off) for rep in (1, 2, 3, 8, 21)
                 for groups, rows, C, ld, off in ((3, 37, 8, 20, 4), (2, 101, 12, 12, 0))]
SUM_REP_BIG = (3, 2, 33001, 128, 132, 4)                           # 2 * 33001 * 32 quads > 2^21


# (name, imgs, (H, W), C, (PH, PW), Ct, nclass)
POOL_CASES = [
    ("vec_Ct4", 6, (23, 31), 8, (4, 6), 4, 3),                     # H % PH = 3, W % PW = 1; Hp = 5 = Wp: see next cases
    ("vec_Ct64", 4, (29, 18), 12, (3, 5), 64, 2),                  # Hp = 9 > Wp = 3
    ("vec_Ct128", 4, (11, 38), 8, (5, 4), 128, 4),                 # Hp = 2 < Wp = 9
    ("vec_Ct256", 6, (14, 9), 4, (4, 2), 256, 3),                  # Hp = 3 < Wp = 4
    ("scalar_C6", 4, (13, 22), 6, (3, 4), 4, 2),                   # C % 4 != 0: scalar kernels
    ("scalar_Ct2", 6, (22, 13), 8, (5, 3), 2, 3),                  # Ct % 4 != 0: scalar kernels; Hp = 4 = Wp
    ("global_Ct0", 5, (13, 21), 16, (13, 21), 0, 1),               # ASPP pooling: (PH, PW) = (H, W), no text
    ("global_Ct0_scalar", 3, (7, 10), 5, (7, 10), 0, 1),
    ("taller_windows", 4, (40, 26), 8, (3, 8), 64, 4),             # Hp = 13 > Wp = 3, PW >= 8: two unrolled quads of columns
]
POOL_BIG = ("two_passes", 4, (130, 133), 128, (4, 3), 0, 1)        # backward: 4 * 130 * 133 * 32 quads > 2^21


def pool_inputs(case):
    name, imgs, (H, W), C, (PH, PW), Ct, nclass = case
    seed = 7000 + sum(map(ord, name))
    Hp, Wp = H // PH, W // PW
    text = _rand((nclass, Ct), seed + 1) if Ct else None
    return _rand((imgs, H, W, C), seed), text, _rand((imgs, Hp, Wp, C + Ct), seed + 2), _rand((imgs, H, W, C), seed + 3)


# (name, imgs, (H, W), C, (KH, KW), dil, pad, gn, ld, off)
COUT1_CASES = [
    ("tiled_C16", 2, (13, 45), 16, (3, 3), 1, 1, False, 24, 4),    # H % 8 = 5, W % 32 = 13
    ("tiled_C32", 3, (21, 37), 32, (3, 3), 1, 1, False, 32, 0),
    ("tiled_C64", 2, (9, 70), 64, (3, 3), 1, 1, False, 72, 8),
    ("tiled_C16_gn", 3, (13, 45), 16, (3, 3), 1, 1, True, 24, 4),
    ("tiled_C32_gn", 2, (21, 37), 32, (3, 3), 1, 1, True, 40, 8),
    ("tiled_C64_gn", 2, (9, 70), 64, (3, 3), 1, 1, True, 64, 0),
    ("generic_dil2", 2, (14, 23), 32, (3, 3), 2, 2, False, 36, 4),
    ("generic_5x3", 2, (11, 19), 8, (5, 3), 1, 1, False, 12, 4),   # pad 1 on a 5-row window: not "same" in y, as the header allows
    ("generic_H5", 3, (5, 41), 32, (3, 3), 1, 1, False, 32, 0),    # H < 8: the tiled kernel does not take it
    ("generic_C4_7x7", 2, (9, 12), 4, (7, 7), 1, 3, False, 8, 4),
]
COUT1_BIG = ("generic_two_passes", 2, (300, 231), 32, (3, 3), 2, 2, False, 32, 0)   # 138600 pixels > 256 * 16 * 32
# weight gradient (3x3 only): the 3x3 cases above and
WGRAD_EXTRA = [
    ("tiny_map_C16", 70, (3, 5), 16, (3, 3), 1, 1, False, 20, 4),  # H W = 15 < PR = 64: the pixel walk wraps several times a step
    ("tiny_map_C16_gn", 70, (3, 5), 16, (3, 3), 1, 1, True, 20, 4),
    ("tiny_map_C4", 100, (2, 3), 4, (3, 3), 1, 1, False, 4, 0),    # PR = 256 = 42 maps and a bit: the row counter wraps 42 times a step
    ("block_edges_gn", 5, (41, 50), 32, (3, 3), 1, 1, True, 32, 0),  # 10250 pixels, 3 blocks of 3417: boundaries inside images
    ("block_edges_dil2", 5, (41, 50), 16, (3, 3), 2, 2, False, 16, 0),
]


def cout1_inputs(case):
    """(x [imgs, H, W, C], wf [KH KW C], bias [1], gn_in [imgs, 2, C] or None, dy [imgs, H, W]) fp32."""
    name, imgs, (H, W), C, (KH, KW), dil, pad, gn, ld, off = case
    seed = 8000 + sum(map(ord, name))
    gn_in = None
    if gn:
        gn_in = torch.stack((0.5 + torch.rand(imgs, C, generator=torch.Generator().manual_seed(seed + 3)),
                             _rand((imgs, C), seed + 4, 0.5)), 1).contiguous()
    return (_rand((imgs, H, W, C), seed), _rand((KH * KW * C,), seed + 1, 0.2), _rand((1,), seed + 2), gn_in,
            _rand((imgs, H, W), seed + 5))


# (name, imgs, (H, W), (KH, KW), dil, pad, sign)
TAP_CASES = [(f"{kh}x{kw}_d{dil}_p{pad}_s{sign:+d}", 2, (13, 22), (kh, kw), dil, pad, sign)
             for (kh, kw, dil, pad) in ((7, 7, 1, 3), (3, 5, 1, 1), (5, 3, 2, 2), (3, 3, 2, 1), (3, 5, 2, 4))
             for sign in (1, -1)]
TAP_BIG = ("3x5_two_passes", 2, (800, 701), (3, 5), 1, 1, -1)      # 1121600 pixels > 256 * 16 * 256


def tap_inputs(case):
    name, imgs, (H, W), (KH, KW), dil, pad, sign = case
    return _rand((imgs, H, W, KH * KW), 9000 + sum(map(ord, name)))


# (name, imgs, (H, W), C, ties)
MAXPOOL_CASES = [
    ("odd_even", 2, (13, 22), 8, False),
    ("even_odd", 2, (22, 13), 12, False),
    ("odd_odd_ties", 3, (9, 15), 4, True),
    ("even_even_ties", 2, (8, 18), 8, True),
    ("one_row", 2, (1, 7), 4, True),
]
MAXPOOL_BIG = ("two_passes", 8, (301, 233), 64, True)              # forward 8 * 151 * 117 * 16 quads > 2^21, backward four times that


def maxpool_inputs(case):
    """(x, dy).  ties: values drawn from five levels, so most windows hold their maximum several times; and one image plane
    constant (every tap ties: the first tap INSIDE the image must win)."""
    name, imgs, (H, W), C, ties = case
    seed = 9500 + sum(map(ord, name))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(imgs, H, W, C, generator=g)
    if ties:
        x = torch.randint(-2, 3, (imgs, H, W, C), generator=g).float()
        x[0, :, :, 0] = -3.0
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return x, torch.randn(imgs, Ho, Wo, C, generator=g)
