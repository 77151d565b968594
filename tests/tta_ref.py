"""Plain float64 restatements of the evaluator's test-time augmentation -- svl_tta_view_f32, svl_tta_accum_f32 and the view
loop of semivl_amd.evaluate.predict(..., tta=...) -- each from the header's formula (include/semivl_hip.h) and the ATen
definition it names, none from the kernels.  Device-agnostic: tests/test_tta_kernels_gpu.py and tests/test_tta_eval_gpu.py
run them on the device, tests/test_tta_ref.py proves them on the CPU against torch's float64 F.interpolate / softmax / flip.

Also here: the DERIVED error bounds, composed from what tests/spatial_ref.py (bilinear_fwd_ref: rounding + coordinate term)
and tests/small_kernel_ref.py (softmax_bound) already derive -- no tolerance is picked -- and the seeded cases both test
files share, so the CPU file can show that torch's own fp32 composition stays inside the bounds on the very inputs the GPU
file uses."""
import numpy as np
import torch

from small_kernel_ref import softmax_bound
from spatial_ref import AGUARD, GUARD, SENTINEL, U, bilinear_fwd_ref, gamma, guard_intact, guarded  # noqa: F401

TTA_GRID_THREADS = 2048 * 256  # threads csrc/tta.hip launches at most (a thread owns 4 columns on the 16-byte path, else 1)


def one_pass():
    return TTA_GRID_THREADS


# ------------------------------------------------------------------------------------------------ view
def view_ref(img, oh, ow, flip):
    """(y, bound) float64: img [..., h, w] -> y [..., oh, ow] = the align_corners = False bilinear resize, with flip mirrored:
    y[..., yy, x] = resized[..., yy, ow - 1 - x].  bound = bilinear_fwd_ref's (rounding + coordinate term) with mirrored columns;
    at oh == h and ow == w every weight is exactly 1 or 0 and the kernel moves the elements: y is the answer to the bit."""
    h, w = img.shape[-2:]
    x = img.double().reshape(-1, h, w, 1)
    y, b = bilinear_fwd_ref(x, oh, ow, False)
    y, b = y.reshape(*img.shape[:-2], oh, ow), b.reshape(*img.shape[:-2], oh, ow)
    return (y.flip(-1), b.flip(-1)) if flip else (y, b)


# ------------------------------------------------------------------------------------------------ accumulate
def interp_ref(src, H, W, align):
    """(u, du) float64 [B, N, H, W]: the bilinear values of every class plane at the target size and bilinear_fwd_ref's bound on
    an fp32 evaluation of each."""
    B, N, h, w = src.shape
    u, du = bilinear_fwd_ref(src.double().reshape(B * N, h, w, 1), H, W, align)
    return u.reshape(B, N, H, W), du.reshape(B, N, H, W)


def scores_ref(u, du, kind):
    """(s, bound) float64 from the interpolated values u and their bounds du (|u~_c - u_c| <= du_c for the fp32 values u~).

    kind 0, s = softmax_c(u): with delta = max_c du_c, softmax(u~)_c / softmax(u)_c = e^{e_c} / sum_k s_k e^{e_k} lies in
    [e^{-2 delta}, e^{2 delta}], so |softmax(u~) - s| <= s (e^{2 delta} - 1); the fp32 evaluation of the softmax itself adds
    small_kernel_ref.softmax_bound, evaluated at the float64 interpolated logits.

    kind 1, s_c = u_c / T, T = sum_k u_k (0 where T == 0).  The fp32 total T^ differs from T by at most
    DT = E + gamma(N) (A + E), E = sum_k du_k, A = sum_k |u_k|: the values' own errors plus an N-term fp32 sum (any order) of
    the fp32 values.  u~_c / T^ - u_c / T = (e_c T - u_c dT) / (T T^) and |T^| >= |T| - DT, so
    |u~_c / T^ - s_c| <= (du_c |T| + |u_c| DT) / (|T| (|T| - DT))   (infinite where DT >= |T|: nothing is claimed there),
    which is the first-order quotient bound (du_c + |s_c| DT) / |T| with its remainder kept; the division's rounding and one
    more of margin add gamma(2) |s_c|: gamma(N) inside DT and this gamma(2) are the N + 2 roundings of the sum, the division
    and the margin.  Where every u_k is 0 in float64 and du is 0 (the taps read only zeros) the kernel's total is exactly 0
    and s = 0 exactly: bound 0."""
    N = u.shape[1]
    if kind == 0:
        delta = du.max(dim=1, keepdim=True).values
        s = u.softmax(dim=1)
        return s, s * torch.expm1(2 * delta) + softmax_bound(u)
    T = u.sum(1, keepdim=True)
    E, A = du.sum(1, keepdim=True), u.abs().sum(1, keepdim=True)
    DT = E + gamma(N) * (A + E)
    zero = (T == 0) & (DT == 0)
    Ts = torch.where(T == 0, torch.ones_like(T), T)
    s = torch.where(T == 0, torch.zeros_like(u), u / Ts)
    room = T.abs() - DT
    b = (du * T.abs() + u.abs() * DT) / (Ts.abs() * room.clamp_min(0)) + gamma(2) * s.abs()
    b = torch.where(room > 0, b, torch.full_like(b, float("inf")))
    return s, torch.where(zero, torch.zeros_like(b), b)


def accum_ref(src, base, H, W, kind, align, flip, scale, interp=None):
    """(out, bound) float64 [B, N, H, W]: out[b, c, y, x] = base[b, c, y, x] + scale * s_c at destination index (y, xs),
    xs = W - 1 - x with flip (base None: not accumulating).  scale is the fp32 value the entry point receives.
    bound = scale * (scores_ref's bound) + gamma(2) (|base| + |scale s| + that): the product and the accumulating sum.
    interp: interp_ref(src, H, W, align) when the caller already has it."""
    u, du = interp if interp is not None else interp_ref(src, H, W, align)
    if flip:
        u, du = u.flip(-1), du.flip(-1)
    s, bs = scores_ref(u, du, kind)
    sc = float(np.float32(scale))
    v, bv = sc * s, abs(sc) * bs
    b0 = torch.zeros_like(v) if base is None else base.double()
    return b0 + v, bv + gamma(2) * (b0.abs() + v.abs() + bv)


# ------------------------------------------------------------------------------------------------ the view loop
def tta_views(ratios, flip):
    return [(r, f) for r in ratios for f in ((False, True) if flip else (False,))]


def predict_tta_ref(single_view, img, H, W, kind, align, ratios, flip):
    """(pred, acc float64 [B, K, H, W], bound): for each ratio in order, unflipped then flipped, the view
    view_ref(img, int(h r + 0.5), int(w r + 0.5), flip) goes through `single_view` (view -> its `final` class map, any float
    dtype; it receives the float64 view cast to img's dtype), and accum_ref adds its scores with scale 1 / n.  pred = argmax
    (first maximum).  bound = the sum of the per-view accum_ref bounds GIVEN each `final` (errors of single_view are not in it)."""
    h, w = img.shape[-2:]
    views = tta_views(ratios, flip)
    acc, bound = None, 0.0
    for r, f in views:
        view = view_ref(img, int(h * r + 0.5), int(w * r + 0.5), f)[0].to(img.dtype)
        acc, b = accum_ref(single_view(view), acc, H, W, kind, align, f, 1.0 / len(views))
        bound = bound + b
    return acc.argmax(dim=1), acc, bound


# ------------------------------------------------------------------------------------------------ shared cases
def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# (name, B, (h, w), (H, W), guard): guard = AGUARD keeps the destination 16-byte aligned, GUARD = 61 puts it 4 bytes past a
# 16-byte boundary (scalar stores whatever W is).
ACCUM_GEOMS = [
    ("identity_5x7", 2, (5, 7), (5, 7), AGUARD),              # odd W: scalar
    ("up4_8x5", 2, (8, 5), (32, 20), AGUARD),                 # W % 4 == 0, aligned: 16-byte stores
    ("down_33x47", 1, (33, 47), (16, 23), AGUARD),            # a reduction, odd W
    ("to_1x1", 2, (3, 4), (1, 1), AGUARD),                    # W = 1
    ("from_1x1", 2, (1, 1), (9, 6), AGUARD),                  # W % 4 == 2
    ("up_frac_6x9_vec", 2, (6, 9), (13, 12), AGUARD),         # fractional ratios, 16-byte stores, rows of 3 quads
    ("up_frac_6x9_off4", 2, (6, 9), (13, 12), GUARD),         # the same 4 bytes off a 16-byte boundary: scalar
]
ACCUM_NS = (1, 2, 19, 21, 150)
# svl_tta_accum_f32 keeps a pixel's N values in LDS with 16-byte stores up to N = 24, with scalar stores up to N = 96, and
# recomputes them beyond: both sides of both thresholds and one N above 256, on a 16-byte geometry and on a scalar one
ACCUM_THRESHOLD_NS = (24, 25, 96, 97, 257)
ACCUM_THRESHOLD_GEOMS = ("up_frac_6x9_vec", "up_frac_6x9_off4")
# N = 2, more work items than one pass of the capped grid: 1025 * 512 quads (16-byte path) and 725 * 725 pixels (scalar)
ACCUM_BIG = [("two_passes_vec", 1, (129, 257), (1025, 2048), AGUARD), ("two_passes_scalar", 1, (91, 90), (725, 725), AGUARD)]
assert 1025 * 512 > one_pass() and 725 * 725 > one_pass()
SCALES = (1.0, 1.0 / 12.0)


def accum_inputs(name, B, N, hw, HW, kind):
    """(src [B, N, h, w], base [B, N, H, W]) fp32, seeded by the case.  kind 0: logits with spreads up to +-30 (a gain of 1, 6
    or 12 by case, clamped).  kind 1: what the sliding-window modes hand over: softmax probabilities times a window count of
    1, 2 or 4 per pixel.  base: a running mean of scores, uniform in [0, 1]."""
    seed = 11000 + sum(map(ord, name)) + 131 * N + 7 * kind
    h, w = hw
    if kind == 0:
        src = (_rand((B, N, h, w), seed) * (1.0, 6.0, 12.0)[seed % 3]).clamp(-30.0, 30.0)
    else:
        cnt = torch.randint(0, 3, (B, 1, h, w), generator=torch.Generator().manual_seed(seed + 1))
        src = (_rand((B, N, h, w), seed) * 3).softmax(1) * (2.0 ** cnt)
    base = torch.rand(B, N, *HW, generator=torch.Generator().manual_seed(seed + 2))
    return src.contiguous(), base


def zero_total_input(N=5):
    """kind 1 source [2, N, 8, 5] whose rows 0-3 x columns 0-2 are zero in every class: resized to (32, 20), the pixels whose
    taps all lie inside that block have a zero total (scores_ref: s = 0, bound 0 there)."""
    src = accum_inputs("zero_total", 2, N, (8, 5), (32, 20), 1)[0]
    src[:, :, :4, :3] = 0.0
    return src.contiguous()


# (name, planes shape, (h, w), (oh, ow))
VIEW_RESIZES = [("half", (2, 3), (37, 50), (19, 25)), ("x1_5", (2, 3), (21, 18), (32, 27)), ("x1_75_vec", (1, 3), (16, 16), (28, 28))]
VIEW_IDENTITY = [("odd", (2, 3), (9, 7)), ("vec", (2, 3), (6, 8))]


def view_input(name, lead, hw):
    return _rand((*lead, *hw), 12000 + sum(map(ord, name))).contiguous()


# ------------------------------------------------------------------------------------------------ the evaluator's toy case
EVAL_K = 5
EVAL_CFG = dict(nclass=EVAL_K, crop_size=32, stride=21)
EVAL_IMG, EVAL_MASK = (2, 3, 75, 90), (80, 96)
EVAL_TTA = dict(ratios=(0.5, 1.0, 1.5), flip=True)
EVAL_MODES = ("original", "zegclip_sliding_window", "sliding_window", "padded_sliding_window")
KIND = {"original": 0, "zegclip_sliding_window": 0, "sliding_window": 1, "padded_sliding_window": 1}


def eval_image(shape=EVAL_IMG, seed=93):
    img = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    return torch.nn.functional.avg_pool2d(img, 5, stride=1, padding=2).contiguous()


def eval_mask(B=EVAL_IMG[0], hw=EVAL_MASK, K=EVAL_K, seed=94):
    m = torch.randint(0, K, (B, *hw), generator=torch.Generator().manual_seed(seed))
    m[:, :3] = 255
    return m
