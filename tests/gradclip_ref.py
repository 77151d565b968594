"""Plain float64 restatement of svl_grad_clip_f32 (include/semivl_hip.h: torch.nn.utils.clip_grad_norm_ over the flat
gradient arena, whose padding is zero), written from the header's formula, with the a-priori bound the GPU tests hold the
kernel to and the seeded value ranges tests/test_gradclip_ref.py (CPU) and tests/test_gradclip_kernels_gpu.py share.  No
tolerance is picked in either.

Bound.  The kernel adds the exact double products g_i^2 (a 24-bit number squared has 48 bits) in double: a sum of n
non-negative terms in ANY order errs by at most (n - 1) u64 relative, u64 = 2^-53 (Higham, Accuracy and Stability of Numerical
Algorithms, section 4.2); the square root halves that and adds one rounding, the products with gscale, the addition of 1e-6
and the division one each: far inside n * 2^-52.  Each of stats[0..2] is then rounded to fp32 ONCE: 2^-24 relative for a
result in fp32's normal range.  So  |out - ref| <= (2^-24 + n * 2^-52) * |ref|.  (The max norm is exact before the one
rounding; the same bound is used.)  A result below fp32's smallest normal number, 2^-126, is rounded to a multiple of 2^-149:
`bound` then carries 2^-150 in place of the 2^-24 term, which is why the tiny-magnitude cases are ALSO run with a power-of-two
gscale that lifts the norm into the normal range, where the relative bound is the whole truth."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
U64X2 = 2.0 ** -52
F32_MIN_NORMAL = 2.0 ** -126


def f32(x):
    """The fp32 number a float argument of the C entry point carries, as a Python float."""
    return float(np.float32(x))


def clip_ref(g, max_norm, norm_type=2.0, gscale=1.0):
    """(norm, coef, scale, nonfinite) in float64 for the arena view `g` (tensor or array of fp32 values):
    norm = gscale * sqrt(sum g^2), or gscale * max |g| for norm_type inf; coef = min(max_norm / (norm + 1e-6), 1), a NaN
    staying a NaN as under torch.clamp; scale = gscale * coef; nonfinite = norm is inf or NaN."""
    a = np.asarray(torch.as_tensor(g).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
    gs, mn = f32(gscale), (math.inf if max_norm == math.inf else f32(max_norm))
    if norm_type in ("inf", math.inf):
        mag = np.abs(a)
        base = float("nan") if np.isnan(mag).any() else (float(mag.max()) if a.size else 0.0)
    else:
        assert float(norm_type) == 2.0, norm_type
        with np.errstate(over="ignore", invalid="ignore"):
            base = math.sqrt(math.fsum(a * a)) if np.isfinite(a).all() else float(np.sqrt(np.sum(a * a)))
    norm = gs * base
    with np.errstate(invalid="ignore"):
        coef = float(np.float64(mn) / np.float64(norm + 1e-6))
    if coef > 1.0:
        coef = 1.0
    return norm, coef, gs * coef, not math.isfinite(norm)


def bound(ref, n):
    """The a-priori bound on |stats[k] - ref| for an arena of n elements (module docstring)."""
    r = abs(ref)
    return (U32 * r if r >= F32_MIN_NORMAL else 2.0 ** -150) + n * U64X2 * r


def relative_bound(ref, n):
    """(2^-24 + n * 2^-52) * |ref|: the bound for results in fp32's normal range."""
    assert abs(ref) >= F32_MIN_NORMAL or ref == 0.0, ref
    return (U32 + n * U64X2) * abs(ref)


# ---- the seeded value ranges -----------------------------------------------------------------------------------------
RANGES = ("normal", "zeros", "huge", "tiny", "nan", "inf")


def values(kind, n, seed):
    """n fp32 values of one of RANGES.  huge: magnitudes from 1e18 to 2.5e19 -- the squares of the larger ones, and any sum of
    a few of the smaller, overflow fp32 while the double sum stays finite; tiny: magnitudes near 1e-40, subnormal in fp32,
    whose squares underflow fp32 to 0; nan / inf: a normal spread with ONE element replaced."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=gen)
    if kind == "zeros":
        return torch.zeros(n)
    if kind == "huge":
        mag = (1.0 + x.abs()) * 1e18
        mag[::3] *= 25.0
        return mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    if kind == "tiny":
        t = ((1.0 + x.abs().double()) * 1e-40 * torch.where(x < 0, -1.0, 1.0).double()).float()
        assert (t != 0).all() and (t.abs() < F32_MIN_NORMAL).all()
        return t
    if kind == "nan":
        x[(2 * n) // 3] = float("nan")
    if kind == "inf":
        x[n // 2] = float("inf")
    return x
