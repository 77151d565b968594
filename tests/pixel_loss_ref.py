"""Float64 restatements, on the CPU, of the unlabelled pixel-loss and label kernels (svl_ce_fused_f32, svl_ce_up_fused_f32,
svl_softmax_max_f32, svl_softmax_max_up_f32, svl_maskclip_labels, svl_concept_max_f32, svl_cutmix_*, svl_count_valid_i64),
the limits the kernels are held to, and the case lists tests/test_pixel_loss_ref.py (CPU) and
tests/test_pixel_loss_kernels_gpu.py (GPU) share.  Everything resized goes through celoss_ref.resize / resize_matrix /
resize_transpose (ATen's upsample_bilinear2d as two dense matrices; the gradient at the head's resolution is the same
matrices transposed).

The criterion (include/semivl_hip.h).  With t the target, t_ok = not (use_ignore_t and t == 255), p = softmax(x),
lse = logsumexp(x), x_l = x[l] for a label l in [0, N) and 0 for any other label (it reads no logit, no one-hot term):
    without conf:  w = 1, valid = t_ok;     with conf:  v = ign != 255, w = 1 if all_pixels else [conf >= conf_thresh and v],
                                                        w *= img_weight[b], valid = v
    sums = { sum t_ok w (lse - x_t),  sum [mc != 255] (lse - x_m),  sum [v] conf,  #valid }
    dlogits = g_t (p - onehot_t) + g_m (p - onehot_m),   g_t = g[0] w where t_ok else 0,  g_m = g[1] where mc != 255 else 0
(conf and conf_thresh are compared as the fp32 numbers the kernel reads.)

LIMITS.  u = 2^-24 (one fp32 rounding, relative); every limit is a first-order count of the roundings of the kernel's own
operations with the constants rounded up, none is fitted to a kernel's output.  N = class count; per pixel X = the largest
|logit| it reads, d_c = max - x_c, E = sum_c p_c d_c (= entropy - log s <= ln N), s = sum_c exp(-d_c) <= N.

(a) Interpolated logit (resized forms), interp_bound.  Tap weights (bilinear_index.h): scale = in / out is one rounding,
    scale (dst + 0.5) - 0.5 two more of numbers below `in`, s - i0 is exact, l0 = 1 - l1 one more: each weight is within
    e = (3 in + 2) u of its float64 value, on either axis (a source coordinate that crosses an integer moves the taps by one
    cell whose weight is then below e: the interpolant is continuous).  Since the two weights of an axis add to 1 (+- u), a
    weight error multiplies the DIFFERENCE of its two taps, at most D = (max - min) of the 2 x 2 cells (+- one cell, for the
    crossing) in that class: (e_y + e_x) D + 2 u X.  Roundings: the staging multiply by the fp32 log2(e) 1.5 u X, the inner
    lx0 a + lx1 b three roundings of numbers <= X, the outer ly0 A + ly1 B three more: 7.5 u X.  Together
        delta = u (c_r X + (3 (h + w) + 4) D),   c_r = 11   (9.5 rounded up for the second-order terms)
    which is the issue's c_r u X with the weight term stated on D <= 2 X so that a common offset of 1000 does not hide the
    labels.  The pixel's delta is the maximum over its classes.
(b) Per-pixel lse - x_t.  Full resolution (two passes): x - m one rounding (relative u of d_c in the exponent), expf 2 u,
    the N-term sum (N - 1) u, so s is within (N + 2 + E) u; logf 2 u log s; m + log s one rounding u |lse|; lse - x_t one
    rounding; the product with w one more: u (|lse| + 2 |lse - x_t| + 2 log s + N + 2 + E) <= u (5 X + N + 2 + 6 ln N)
        <= u (c_1 X + c_2 (N + k)),   c_1 = 5, c_2 = 2, k = 8        (N + 16 >= 6 ln N + 2 for every N >= 1)
    Resized (base 2, online): each of at most N steps is one v_exp_f32 (2 u) and one fused multiply-add (u), the exponents'
    roundings telescope to d_c u: s within (3 N + E) u; log2 2 u; m + log2 s u |lse|; lse - x_t u; times the fp32 ln 2
    1.5 u; times w u; and both lse and x_t carry delta:
        <= u (c_1 X + c_2 (N + k)) + 2 delta,   c_1 = 8, c_2 = 4, k = 8   (|lse| + 3.5 |lse - x_t| + 3 N + 3 ln N)
(c) conf and p_c, relative (the form of small_kernel_ref.softmax_bound: (|x_c - max| + c N + k) u).
    Full-resolution CE: e_c (d_c + 2) u, s (N + 2 + E) u, 1 / s and the product 2 u: (d_c + E + N + 6) u.  The limit
    used is (2 d_c + E + N + 6) u: it also admits the other fp32 route to the same number, exp(x_c - m - log s), whose two
    subtractions each round a number of size d_c (torch's log_softmax; the CPU test holds torch's fp32 to these limits).
    The second d_c matters only where p_c is tiny.
    Softmax-max (online with expf: one expf, one multiply-add per step): s within (3 N + E) u, the reciprocal u; conf is the
    class with d_c = 0: (E + 3 N + 6) u -- and, resized, times exp(2 delta).
    Resized CE: p_c = exp2(x_c - lse) with lse as in (b): lse within (3 N + E + 2 ln N) u + u |lse|, the subtraction
    (d_c + ln N) u, exp2 2 u: (X + d_c + E + 3 N + 4 ln N + 6) u, times exp(2 delta); used with 2 d_c like the one above.
(d) Gradient element: G = g_t + g_m (one rounding; g_t = g[0] w one more), G p_c one, each one-hot subtraction one:
        G (p_c rel(p_c) + 2^-126) + 4 u (G p_c + g_t [c = t] + g_m [c = m]) + 2^-126
    (the absolute terms, as in softmax_bound, cover probabilities and products below the normal range, which are flushed).
    At the head's resolution the kernel gathers sum w32 d32 over a cell's footprint with weights within e of the float64
    ones (also next to their support: the crossing) and at most 24 roundings per term (w_x = the sum of two tap weights,
    w_x d, ten column adds, w_y, w_y r, at most ten row adds): with T+ the transpose with weights w + e
        T+(|d| + bound) (1 + 24 u) - T(|d|).
    Sum over the classes (exactly 0 in float64): the fp32 p_c add up to 1 within (N + 2) u (full resolution: the same e_c
    the sum s was formed from) or (X + 3 N + 2 E + 4 ln N + 2) u (resized: exp2(x_c - lse), the lse of (c)), plus 3 u of
    roundings on each of G, g_t, g_m:  <= 2 G u (N + 8)  resp.  2 G u (X + 3 N + 6 ln N + 8); the resized one goes through T+
    (the weights do not depend on the class) plus the gather's 24 u sum_c |d_c|.
(e) Block sums: fp32 partial sums of at most 256 pixels (a six-level shuffle tree and four waves: 8 additions on any path)
    or 40 x 40 pixels (at most 4 per thread, the tree, eight waves: 18), then double (2^-53: nothing).  Every term of one
    sign: 10 u sum |term| resp. 20 u sum |term| on top of the sum of the per-pixel bounds.  #valid is an exact integer.
"""
import math

import torch

from celoss_ref import resize, resize_matrix, resize_transpose  # noqa: F401  (re-exported)

IGNORE = 255
U = 2.0 ** -24
C_R = 11.0
GATHER_ROUNDINGS = 24
TREE_FULL, TREE_UP = 10, 20


def _d(x):
    return x.detach().double().cpu()


def f32(v):
    """The fp32 number a kernel reads for the Python float v."""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ the plain criterion
def _pick(xs, lab, N):
    inr = (lab >= 0) & (lab < N)
    li = torch.where(inr, lab, torch.zeros_like(lab))
    xl = torch.where(inr, xs.gather(-1, li.unsqueeze(-1)).squeeze(-1), torch.zeros((), dtype=torch.float64))
    return xl, torch.nn.functional.one_hot(li, N).double() * inr.unsqueeze(-1)


def ce_plain(x, target, use_ignore_t=True, conf=None, ign=None, conf_thresh=0.0, all_pixels=False, img_weight=None, mc=None,
             g=(0.0, 0.0)):
    """x [B, N, *], maps [B, *] -> dict of float64 CPU tensors: sums [4], grad [B, N, *], and the per-pixel quantities the
    limits are made of (lse, p [B, *, N], d = max - x, ce_t, ce_m, sc, gt, gm, oht, ohm)."""
    x = _d(x)
    B, N = x.shape[:2]
    xs = x.movedim(1, -1)
    t = target.detach().cpu()
    zero = torch.zeros((), dtype=torch.float64)
    lse = torch.logsumexp(xs, -1)
    p = torch.softmax(xs, -1)
    t_ok = (t != IGNORE) if use_ignore_t else torch.ones_like(t, dtype=torch.bool)
    w = torch.ones_like(lse)
    valid, sc = t_ok, torch.zeros_like(lse)
    if conf is not None:
        v = ign.detach().cpu() != IGNORE
        cf = conf.detach().float().cpu().double()
        w = torch.ones_like(lse) if all_pixels else ((cf >= f32(conf_thresh)) & v).double()
        if img_weight is not None:
            w = w * _d(img_weight.float()).view(B, *([1] * (t.dim() - 1)))
        valid, sc = v, torch.where(v, cf, zero)
    else:
        assert ign is None and img_weight is None, "refused by the entry points"
    xt, oht = _pick(xs, t, N)
    ce_t = torch.where(t_ok, w * (lse - xt), zero)
    if mc is not None:
        m = mc.detach().cpu()
        m_ok = m != IGNORE
        xm, ohm = _pick(xs, m, N)
        ce_m = torch.where(m_ok, lse - xm, zero)
    else:
        m_ok, ohm, ce_m = torch.zeros_like(t_ok), torch.zeros_like(oht), torch.zeros_like(lse)
    gt = torch.where(t_ok, float(g[0]) * w, zero) if bool(t_ok.any()) else torch.zeros_like(lse)
    gm = torch.where(m_ok, torch.full_like(lse, float(g[1])), zero)
    grad = gt.unsqueeze(-1) * (p - oht) + gm.unsqueeze(-1) * (p - ohm)
    sums = torch.stack([ce_t.sum(), ce_m.sum(), sc.sum(), valid.sum().double()])
    return dict(sums=sums, grad=grad.movedim(-1, 1).contiguous(), lse=lse, p=p, d=xs.amax(-1, keepdim=True) - xs, ce_t=ce_t,
                ce_m=ce_m, sc=sc, gt=gt, gm=gm, oht=oht, ohm=ohm, X=xs.abs().amax(-1), N=N, w_eff=torch.where(t_ok, w, zero),
                m_ok=m_ok.double())


def ce_plain_up(x, H, W, align, target, **kw):
    """ce_plain on resize(x [B, N, h, w]); `grad` is carried to x's own resolution, `grad_full` stays at [H, W]."""
    out = ce_plain(resize(x, H, W, align), target, **kw)
    out["grad_full"] = out["grad"]
    out["grad"] = resize_transpose(out["grad_full"], x.shape[2], x.shape[3], align)
    return out


# ------------------------------------------------------------------------------------------------ limits
def _axis_windows(n_in, n_out, align):
    """[n_out, n_in] bool: the two taps of every destination index, widened by one cell on either side."""
    sup = resize_matrix(n_in, n_out, align) > 0
    wide = sup.clone()
    wide[:, 1:] |= sup[:, :-1]
    wide[:, :-1] |= sup[:, 1:]
    return wide


def _window_reduce(a, my, mx, op):
    """a [..., h, w] -> [..., H, W]: op (amax / amin) over the rectangular window my[Y] x mx[X]."""
    fill = -math.inf if op == "amax" else math.inf
    t = torch.where(my.view(*([1] * (a.dim() - 2)), my.shape[0], my.shape[1], 1), a.unsqueeze(-3), torch.full((), fill, dtype=a.dtype))
    t = getattr(t, op)(-2)                                                         # [..., H, w]
    t = torch.where(mx.view(*([1] * (a.dim() - 2)), 1, mx.shape[0], mx.shape[1]), t.unsqueeze(-2), torch.full((), fill, dtype=a.dtype))
    return getattr(t, op)(-1)                                                      # [..., H, W]


def interp_bound(x, H, W, align):
    """(delta [B, H, W], X [B, H, W]) of (a): the bound on every interpolated logit of a pixel and the largest |logit| it reads."""
    x = _d(x)
    h, w = x.shape[2:]
    my, mx = _axis_windows(h, H, align), _axis_windows(w, W, align)
    hi, lo = _window_reduce(x, my, mx, "amax"), _window_reduce(x, my, mx, "amin")
    X = torch.maximum(hi.abs(), lo.abs()).amax(1)
    D = (hi - lo).amax(1)
    return U * (C_R * X + (3 * (h + w) + 4) * D), X


def _axis_plus(n_in, n_out, align):
    """resize_matrix with every weight on or next to the support raised by e = (3 in + 2) u."""
    return resize_matrix(n_in, n_out, align) + (3 * n_in + 2) * U * _axis_windows(n_in, n_out, align).double()


def transpose_plus(bfull, h, w, align):
    """T+ of (d): the resize's transpose with the weights w + e, for non-negative [B, N, H, W] (or [B, H, W]) maps."""
    squeeze = bfull.dim() == 3
    b = bfull.unsqueeze(1) if squeeze else bfull
    ry, rx = _axis_plus(h, b.shape[2], align), _axis_plus(w, b.shape[3], align)
    out = torch.einsum("Yy,bnYX,Xx->bnyx", ry, b.double(), rx)
    return out[:, 0] if squeeze else out


def ce_bounds(ref, up=None):
    """Limits (b) - (e) for a result of ce_plain (up = None) or ce_plain_up (up = (x, H, W, align)): dict with sums [4]
    (absolute; [3] is 0: exact), grad (elementwise, at the resolution of ref['grad']) and rowsum (|sum over classes|)."""
    N = ref["N"]
    p, d = ref["p"], ref["d"]
    E = (p * d).sum(-1, keepdim=True)
    lnN = math.log(N)
    if up is None:
        X = ref["X"]
        pix = U * (5 * X + 2 * (N + 8))
        rel = U * (2 * d + E + N + 6)
        rows = 2 * U * (N + 8)
        tree = TREE_FULL
    else:
        x, H, W, align = up
        delta, Xl = interp_bound(x, H, W, align)
        X = torch.maximum(Xl, ref["X"])
        pix = U * (8 * X + 4 * (N + 8)) + 2 * delta
        e2 = torch.exp(2 * delta).unsqueeze(-1)
        rel = (1 + U * (X.unsqueeze(-1) + 2 * d + E + 3 * N + 4 * lnN + 6)) * e2 - 1
        rows = 2 * U * (X + 3 * N + 6 * lnN + 8)
        tree = TREE_UP
    s0 = (ref["w_eff"] * pix).sum() + tree * U * ref["ce_t"].abs().sum()
    s1 = (ref["m_ok"] * pix).sum() + tree * U * ref["ce_m"].abs().sum()
    s2 = tree * U * ref["sc"].abs().sum()
    G = (ref["gt"] + ref["gm"]).unsqueeze(-1)
    gfull = 2.0 ** -126 + G * (p * rel + 2.0 ** -126) + 4 * U * (G * p + ref["gt"].unsqueeze(-1) * ref["oht"] + ref["gm"].unsqueeze(-1) * ref["ohm"])
    gfull = gfull.movedim(-1, 1)
    rowsum = G.squeeze(-1) * rows
    if up is None:
        return dict(sums=torch.stack([s0, s1, s2, torch.zeros(())]), grad=gfull, rowsum=rowsum)
    h, w = x.shape[2:]
    absd = ref["grad_full"].abs()
    glow = transpose_plus(absd + gfull, h, w, align) * (1 + GATHER_ROUNDINGS * U) - resize_transpose(absd, h, w, align)
    rowlow = transpose_plus(rowsum, h, w, align) + GATHER_ROUNDINGS * U * transpose_plus(absd.sum(1), h, w, align)
    return dict(sums=torch.stack([s0, s1, s2, torch.zeros(())]), grad=glow, rowsum=rowlow, grad_full=gfull, delta=delta)


# ------------------------------------------------------------------------------------------------ softmax-max
def softmax_max(x):
    """x [B, N, *] -> (conf, label of the first maximum, float64 gap between the two largest logits; inf at N = 1)."""
    x = _d(x)
    conf = torch.softmax(x, 1).amax(1)
    cls = torch.arange(x.shape[1]).view(1, -1, *([1] * (x.dim() - 2)))
    first = torch.where(x == x.amax(1, keepdim=True), cls, torch.full_like(cls, x.shape[1])).amin(1)
    if x.shape[1] > 1:
        top = x.topk(2, dim=1).values
        gap = top[:, 0] - top[:, 1]
    else:
        gap = torch.full_like(conf, math.inf)
    return conf, first, gap


def softmax_max_up(x, H, W, align):
    return softmax_max(resize(x, H, W, align))


def conf_bound(xfull, delta=None):
    """(c): the absolute limit on conf of softmax-max, [B, *]."""
    x = _d(xfull)
    N = x.shape[1]
    p = torch.softmax(x, 1)
    E = (p * (x.amax(1, keepdim=True) - x)).sum(1)
    rel = U * (E + 3 * N + 6)
    if delta is not None:
        rel = (1 + rel) * torch.exp(2 * delta) - 1
    return p.amax(1) * rel + 2.0 ** -126


# ------------------------------------------------------------------------------------------------ label kernels
def maskclip_labels(dense, H, W, scale, thresh, ign=None):
    """MaskCLIP's label tail: resize (align_corners = False, any geometry) -> softmax(scale x) -> max -> 255 where
    conf < thresh or ign == 255.  Returns (label, |conf - thresh|, top-2 gap of the scaled logits, bound on the scaled
    logits, bound on conf): labels are compared where gap > 2 zbound and |conf - thresh| > cbound."""
    v = resize(dense, H, W, False)
    z = float(scale) * v
    conf, idx, gap = softmax_max(z)
    delta, X = interp_bound(dense, H, W, False)
    zb = abs(float(scale)) * (delta + 2 * U * X)                 # the product with the fp32 scale: its rounding and the scale's
    cb = conf_bound(z, zb)
    label = torch.where(conf < f32(thresh), torch.full_like(idx, IGNORE), idx)
    if ign is not None:
        label = torch.where(ign.cpu() == IGNORE, torch.full_like(idx, IGNORE), label)
    return label, (conf - f32(thresh)).abs(), gap, zb, cb


def concept_max(pred, offsets, N):
    """pred [B, NC, *] -> [B, N, *]: the maximum over each concept's classes off[c] .. off[c + 1]."""
    off = [int(o) for o in offsets]
    return torch.stack([pred[:, off[c]:off[c + 1]].amax(1) for c in range(N)], 1)


def cutmix(a, b, box):
    """where(box == 1, b, a); box [B, *] broadcast over the channels of a, b [B, C, *] (or no channel axis)."""
    m = box == 1.0
    if a.dim() == box.dim() + 1:
        m = m.unsqueeze(1)
    return torch.where(m, b, a)


def count_valid(m):
    return int((m != IGNORE).sum().item())


# ------------------------------------------------------------------------------------------------ shared cases
# (B, N, HW): HW < P, HW = P + 4 (a second block of one float4), odd HW (the scalar path), and every tile width on both
# sides of its switch (ce_tile_pixels: P = 256 up to N = 64, 128 up to 128, 64 up to 256: 1, 2, 4 threads per pixel)
FUSED_SHAPES = [(2, 1, 37), (1, 2, 1), (2, 21, 672), (1, 64, 260), (1, 65, 300), (2, 128, 132), (1, 129, 68), (1, 256, 70),
                (3, 19, 1031)]
# (N, h, w, H, W) of the resize-fused kernels (tiles of 8 x 8 cells, at most 40 resized rows / columns per tile, ratio <= 4.5,
# N <= 160).  Chosen with the host-only query svl_ce_up_num_blocks (tests/test_pixel_loss_ref.py asserts what it answers):
UP_GEOMS = [
    (5, 8, 8, 32, 32),        # exactly one tile, ratio 4
    (7, 13, 20, 50, 79),      # ragged tiles, non-integer ratios that differ between the axes
    (3, 9, 9, 9, 9),          # ratio 1; a last tile of one cell on both axes
    (4, 17, 11, 34, 22),      # ratio 2; a last tile of one cell (rows)
    (2, 2, 3, 9, 13),         # fewer cells than a tile edge; 2 -> 9 and 3 -> 13: the largest `out` the query accepts
    (2, 2, 3, 5, 10),         # 2 -> 5 and 3 -> 10: the largest with align_corners (taken without it as well)
    (3, 7, 9, 7, 36),         # ratio 1 on the rows, 4 on the columns; 7 cells (under a tile), 9 (one cell left over)
    (6, 17, 8, 76, 8),        # the largest `out` at in = 17 (ratio 4.47, regions of 40 rows), ratio 1 on the columns
    (6, 17, 8, 73, 8),        # its largest with align_corners (taken without it as well)
    (160, 16, 16, 72, 72),    # N = 160 = UP_MAX_N at ratio 4.5, the largest regions: the 160 KB of LDS would hold N = 177 at
    (160, 16, 16, 68, 68),    # a 40 x 40 region, so the largest N the LDS allows there is the largest N there is
    (160, 2, 2, 2, 2),        # N = 160 at the smallest region
]
# geometries the query accepts with one value of align_corners only (the other one is refused: test_geometry_queries of the GPU test asserts both)
UP_ONLY_ALIGN = {(2, 2, 3, 9, 13): False, (6, 17, 8, 76, 8): False, (160, 16, 16, 72, 72): False}
# (N, h, w, H, W, align) the query refuses: N = 161, and one past the largest `out` of an axis
UP_REFUSED = [(161, 2, 2, 2, 2, False), (161, 2, 2, 2, 2, True), (2, 2, 3, 10, 13, False), (2, 2, 3, 9, 14, False),
              (2, 2, 3, 6, 10, True), (6, 17, 8, 77, 8, False), (6, 17, 8, 74, 8, True)]
VALUE_CASES = ["baseline", "x30", "plus1000", "minus1000", "dominant", "equal", "twin"]


def logits(case, shape, seed):
    """fp32 logits [B, N, ...] of a value case: randn x 2; randn x 30; randn x 2 +- 1000 (a common offset); one dominant
    class per pixel with a gap >= 60; all logits equal; two bit-identical class planes above the rest (first index wins)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * 2
    N = shape[1]
    if case == "baseline":
        return x
    if case == "x30":
        return x * 15
    if case == "plus1000":
        return x + 1000
    if case == "minus1000":
        return x - 1000
    if case == "dominant":
        return x          # case_inputs raises class (b + 1) % N of image b by 80 on every pixel (the resized forms keep the gap)
    if case == "equal":
        return torch.full(shape, 3.25)
    if case == "twin":
        if N >= 2:
            a, b = (N // 3) % N, N - 1
            if a == b:
                a = 0
            x[:, a] = x[:, a].abs() + 20
            x[:, b] = x[:, a]
        return x
    raise KeyError(case)


def dominant_class(b, N):
    return (b + 1) % N


def maps(shape_t, N, seed, n_at_thresh=300, conf_thresh=0.7):
    """The maps of the descriptor forms, on a [B, *] grid: target (about 10 % of it 255, a fully ignored band in image 0),
    lab (no 255), conf (rand; a few hundred set exactly to fp32(conf_thresh)), ign (a band of 255 in image 0, the whole of the
    last image when B > 1), mc (half of it 255)."""
    g = torch.Generator().manual_seed(seed)
    B = shape_t[0]
    n = 1
    for s in shape_t[1:]:
        n *= s
    lab = torch.randint(0, N, shape_t, generator=g)
    t = lab.clone()
    t[torch.rand(*shape_t, generator=g) < 0.1] = IGNORE
    band = slice(0, max(1, min(32, n // 2)))
    t.view(B, -1)[0, band] = IGNORE
    conf = torch.rand(*shape_t, generator=g)
    k = min(n_at_thresh, max(1, (B * n) // 3))
    conf.view(-1)[torch.randperm(B * n, generator=g)[:k]] = f32(conf_thresh)
    ign = torch.zeros(shape_t, dtype=torch.int64)
    ign.view(B, -1)[0, n // 3:n // 3 + max(1, n // 5)] = IGNORE
    if B > 1:
        ign[B - 1] = IGNORE
    mc = torch.randint(0, N, shape_t, generator=g)
    mc[torch.rand(*shape_t, generator=g) < 0.5] = IGNORE
    return dict(target=t, lab=lab, conf=conf, ign=ign, mc=mc)


FORMS = ["supervised", "pixelwise0.0", "pixelwise0.7", "pixelwise1.0", "guided", "all_pixels"]


def form_kwargs(form, m, B):
    """(target, keyword arguments of ce_plain / ops.ce_fused without g) of a descriptor form on maps m."""
    if form == "supervised":
        return m["target"], dict(use_ignore_t=True)
    if form.startswith("pixelwise"):
        th = float(form[len("pixelwise"):])
        conf = m["conf"].clone()
        conf[conf == f32(0.7)] = f32(th)          # the confidences at the threshold move with it
        return m["lab"], dict(use_ignore_t=False, conf=conf, ign=m["ign"], conf_thresh=th)
    if form == "guided":
        return m["lab"], dict(use_ignore_t=False, conf=m["conf"], ign=m["ign"], conf_thresh=0.7, mc=m["mc"])
    if form == "all_pixels":
        iw = torch.linspace(0.25, 0.75, B) if B > 1 else torch.tensor([0.375])
        return m["lab"], dict(use_ignore_t=False, conf=m["conf"], ign=m["ign"], conf_thresh=0.7, all_pixels=True, img_weight=iw)
    raise KeyError(form)


def form_gscale(form, n):
    """The two fp32 gradient scales of a form on n pixels (g_m != 0 only with a guidance map)."""
    return (f32(0.125 / n), f32(0.03 / n) if form == "guided" else 0.0)


def up_pairs():
    """Every (geometry, align_corners) of UP_GEOMS the kernels take."""
    return [(g, a) for g in UP_GEOMS for a in (False, True) if UP_ONLY_ALIGN.get(g, a) == a]


def case_forms():
    """(value case, descriptor form): every form on the baseline values, the supervised and the guided one on the others."""
    return [("baseline", f) for f in FORMS] + [(c, f) for c in VALUE_CASES[1:] for f in ("supervised", "guided")]


def case_inputs(case, shape_x, shape_t, seed):
    """(logits, maps) of a value case.  'dominant': the target is the dominant class on every other pixel and another class
    on the rest."""
    N = shape_x[1]
    x = logits(case, shape_x, seed)
    m = maps(shape_t, N, seed + 1)
    if case == "dominant":
        x.clamp_(-10, 10)
        for b in range(shape_x[0]):
            x[b, dominant_class(b, N)] += 80
            dom = dominant_class(b, N)
            for k in ("lab", "target"):
                flat = m[k][b].view(-1)
                keep = flat == IGNORE
                off = torch.where(flat == dom, torch.full_like(flat, (dom + 1) % N), flat)
                flat.copy_(torch.where(torch.arange(flat.numel()) % 2 == 0, torch.full_like(flat, dom), off))
                flat[keep] = IGNORE
    return x, m


def ratio(err, bound):
    """max of err / bound; 0 where err is exactly 0; inf where err is NaN or the bound is 0 and the error is not."""
    err, bound = err.double(), torch.as_tensor(bound, dtype=torch.float64)
    r = torch.where(err == 0, torch.zeros((), dtype=torch.float64), err / bound)
    r = torch.where(torch.isnan(r), torch.full((), math.inf, dtype=torch.float64), r)
    return float(r.max()) if r.numel() else 0.0


def ce_ratios(sums, grad, ref, bnd):
    """error / limit of a result (sums [4], grad or None) against a reference and its ce_bounds: dict sum0, sum1, sum2,
    count (0 or inf: exact), grad, rowsum (the gradient's sum over the classes)."""
    sums = sums.double().cpu()
    out = {f"sum{k}": ratio((sums[k] - ref["sums"][k]).abs(), bnd["sums"][k]) for k in range(3)}
    out["count"] = 0.0 if sums[3].item() == ref["sums"][3].item() else math.inf
    if grad is not None:
        g = grad.double().cpu()
        out["grad"] = ratio((g - ref["grad"]).abs(), bnd["grad"])
        # (the reference's own sum is 0 up to its float64 rounding, except on a label outside [0, N): g p has no one-hot term)
        out["rowsum"] = ratio((g.sum(1) - ref["grad"].sum(1)).abs(), bnd["rowsum"])
    return out


def maskclip_cases():
    """(name, dense, H, W, thresh, ign): scale 100 on cosine-like values.  thresh 1.0 is run on small values (no confidence
    rounds to 1: every label is 255) and on a constant N = 1 map (conf is exactly 1: label 0)."""
    g = torch.Generator().manual_seed(77)
    d = torch.randn(2, 5, 8, 8, generator=g) * 0.05
    ign = torch.zeros(2, 29, 31, dtype=torch.int64)
    ign[0, 5:9] = 255
    ign1 = ign.clone()
    ign1[1] = 255
    return [("up_noign_0.9", d, 29, 31, 0.9, None), ("up_band_0.9", d, 29, 31, 0.9, ign), ("up_image_0.0", d, 29, 31, 0.0, ign1),
            ("up_1.0", d * 0.2, 29, 31, 1.0, None), ("down_0.9", torch.randn(1, 4, 16, 12, generator=g) * 0.05, 7, 5, 0.9, None),
            ("ratio1_0.5", torch.randn(2, 3, 9, 9, generator=g) * 0.05, 9, 9, 0.5, None),
            ("N1", torch.randn(2, 1, 5, 6, generator=g) * 0.05, 11, 13, 1.0, None),
            ("const_tie", torch.full((1, 4, 6, 6), 0.125), 13, 17, 0.25, None)]


def tie_first(case, N):
    """The exact label of a constructed tie ('equal', 'twin' of logits()): the first index among the maxima."""
    if case == "equal" or N < 2:
        return 0
    a = (N // 3) % N
    return 0 if a == N - 1 else a
