"""Plain float64 restatements of the ROW half of csrc/norm.hip -- LayerNorm (svl_layernorm_fwd / _fwd_planes / _fwd_planes_f16x2 /
_bwd), the row softmax (svl_softmax_rows_fwd / _bwd), the L2 normalisation (svl_l2norm_fwd / _bwd), the column sums
(svl_colsum_f32) and the exact movers (svl_chanmask_f32, svl_permute_rows_f32, svl_bound2_f32) -- each from the formulas of
include/semivl_hip.h and the semantics of F.layer_norm / softmax / F.normalize, none from the kernels.  Device-agnostic, like
tests/imgnorm_ref.py, whose SECOND convention and (through tests/spatial_ref.py) strided / guard-band helpers and unit
roundoff it reuses: tests/test_rownorm_kernels_gpu.py runs them on the device, tests/test_rownorm_ref.py proves them on the CPU
against ATen float64 and autograd.

Every restatement returns (want, bound).  `bound` is a running error bound, element by element, of an fp32 evaluation of the
header's formula.  A quantity travels as a pair (v, e): v its exact float64 value, e a bound of the error of ANY fp32
evaluation so far.  Each operation carries the operands' errors through with its partial derivatives and adds its own rounding:
  rounding          U = 2^-24 times the magnitude of the computed result, |v| + e
  a b               |a| eb + |b| ea + ea eb          (the product of the two errors is kept: a centred value x - mean can be
                                                      far smaller than its error when the mean is 100 standard deviations)
  sum of n terms    sum e_i + n U sum (|t_i| + e_i)  in ANY order: an addition with an exactly zero operand is exact and every
                                                      other one merges two groups of non-zero terms, so no term passes more
                                                      than n - 1 roundings, n = the NON-ZERO terms
  sqrtf, 1 / x, x / C, expf     one ulp = 2 U (the figure tests/small_kernel_ref.softmax_bound uses for the device functions),
                                their operand's error through the exact change of the function over [v - e, v + e]
  results that may fall below the normal range (expf of a large negative number, the square of a 1e-20 value, a product with
  such an exponential) add TINY = 2^-126, whether the device flushes them or rounds them to a subnormal.
What is left is the compounding of the roundings of a sum, (1 + U)^n - 1 - n U <= n U 2^-10 while n <= 16384 (asserted):
the factor SECOND = 1 + 2^-10 on every bound.  No tolerance is chosen anywhere; eps and scale enter at their fp32 values.
A bound of exactly 0 (gamma = beta = 0, the padding of a softmax row, dx where dy = 0, the y of a zero row) means equality.

Also here: the seeded case lists and input builders both test files share."""
import functools

import numpy as np
import torch

from imgnorm_ref import SECOND, f32
from spatial_ref import AGUARD, SENTINEL, U, gaps_intact, guard_intact, guarded, strided  # noqa: F401  (re-exported)

TINY = 2.0 ** -126                   # smallest normal fp32 number
ULP = 2.0 * U                        # sqrtf, division, expf: within one ulp
MAX_TERMS = 16384                    # n U <= 2^-10: see the module docstring


# ------------------------------------------------------------------------------------------------ the (value, error) calculus
def _c(t):
    """An exact operand (an fp32 input): (float64 value, zero error)."""
    v = t.double()
    return v, torch.zeros_like(v)


def _rnd(v, e, k=U):
    return v, e + k * (v.abs() + e)


def _add(a, b):
    return _rnd(a[0] + b[0], a[1] + b[1])


def _sub(a, b):
    return _rnd(a[0] - b[0], a[1] + b[1])


def _mul(a, b, tiny=False):
    v, e = _rnd(a[0] * b[0], a[0].abs() * b[1] + b[0].abs() * a[1] + a[1] * b[1])
    return (v, e + TINY * (v != 0)) if tiny else (v, e)


def _sum(a, dim):
    n = ((a[0] != 0) | (a[1] != 0)).sum(dim, keepdim=True)
    assert int(n.max()) <= MAX_TERMS
    return a[0].sum(dim, keepdim=True), a[1].sum(dim, keepdim=True) + n * U * (a[0].abs() + a[1]).sum(dim, keepdim=True)


def _divc(a, c):
    return _rnd(a[0] / c, a[1] / c, ULP)


def _sqrt(a):
    v = torch.sqrt(a[0])
    lo = torch.sqrt((a[0] - a[1]).clamp_min(0.0))
    e = torch.where(a[1] > 0, a[1] / (v + lo).clamp_min(1e-300), torch.zeros_like(v))
    return _rnd(v, e, ULP)


def _recip(a):
    assert bool((a[0].abs() > a[1]).all()), "1 / x: the error bound of x reaches x"
    return _rnd(1.0 / a[0], a[1] / (a[0].abs() * (a[0].abs() - a[1])), ULP)


def _exp(a):
    v = torch.exp(a[0])
    v, e = _rnd(v, v * torch.expm1(a[1]), ULP)
    return v, e + TINY


def _out(a):
    return a[0], SECOND * a[1]


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd_ref(x, gamma, beta, eps, divisor=None, eps_outside=False, mean_drops_quad=False):
    """x [rows, C] -> dict y / dy_ [rows, C], stats / dstats [rows, 2] = (mean, rstd), float64 values and bounds:
      mean = sum(x) / C;  var = sum((x - mean)^2) / C (two passes, biased);  rstd = 1 / sqrt(var + eps);
      y = ((x - mean) rstd) gamma + beta                        (the header's order, one rounding per operation).
    The keyword arguments are the seeded MUTATIONS of tests/test_rownorm_ref.py: divisor (C - 1 under the variance),
    eps_outside (1 / (sqrt(var) + eps)), mean_drops_quad (the last four channels left out of the sum under the mean)."""
    C = x.shape[1]
    X, G, B = _c(x), _c(gamma[None, :]), _c(beta[None, :])
    mean = _divc(_sum((X[0][:, :-4], X[1][:, :-4]) if mean_drops_quad else X, 1), C)
    a = _sub(X, mean)
    q = _mul(a, a)
    var = _divc(_sum((q[0], q[1] + TINY), 1), C if divisor is None else divisor)
    E = _c(torch.tensor(f32(eps), dtype=torch.float64, device=x.device))
    s = _sqrt(_add(var, E))
    if eps_outside:                  # (only a mutation's values are used: a constant row's sqrt(var) carries an error above eps)
        s = (torch.sqrt(var[0]) + E[0], torch.zeros_like(s[1]))
    rstd = _recip(s)
    y = _add(_mul(_mul(a, rstd), G), B)
    return dict(y=y[0], dy_=SECOND * y[1], stats=torch.cat((mean[0], rstd[0]), 1), dstats=SECOND * torch.cat((mean[1], rstd[1]), 1))


def ln_bwd_ref(dy, x, stats, gamma, dx_add=None, drop_m2=False, drop_row=None):
    """LayerNorm backward of the header from the statistics it is GIVEN (stats [rows, 2], exact operands: the kernel reads them):
      xhat = (x - mean) rstd;  g = dy gamma;  m1 = sum_c g / C;  m2 = sum_c (g xhat) / C;
      dx = rstd ((g - m1) - xhat m2) (+ dx_add);   dgamma = sum_r dy xhat,  dbeta = sum_r dy.
    dict dx / ddx, dgamma / ddgamma, dbeta / ddbeta.  MUTATIONS: drop_m2 (the xhat m2 term), drop_row (that row left out of
    dgamma and dbeta); dx_add dropped is simply dx_add=None."""
    C = x.shape[1]
    st = stats.double()
    mean, rstd = (st[:, 0:1], torch.zeros_like(st[:, 0:1])), (st[:, 1:2], torch.zeros_like(st[:, 1:2]))
    X, D, G = _c(x), _c(dy), _c(gamma[None, :])
    xh = _mul(_sub(X, mean), rstd)
    g = _mul(D, G)
    m1 = _divc(_sum(g, 1), C)
    t = _sub(g, m1)
    if not drop_m2:
        t = _sub(t, _mul(xh, _divc(_sum(_mul(g, xh), 1), C)))
    dx = _mul(rstd, t)
    if dx_add is not None:
        dx = _add(dx, _c(dx_add))
    pg, pb = _mul(D, xh), D
    if drop_row is not None:
        keep = torch.ones(x.shape[0], 1, dtype=torch.float64, device=x.device)
        keep[drop_row] = 0.0
        pg, pb = (pg[0] * keep, pg[1] * keep), (pb[0] * keep, pb[1] * keep)
    dg, db = _sum(pg, 0), _sum(pb, 0)
    return dict(dx=dx[0], ddx=SECOND * dx[1], dgamma=dg[0][0], ddgamma=SECOND * dg[1][0], dbeta=db[0][0], ddbeta=SECOND * db[1][0])


def sexp_ref(y):
    """int32 [rows]: the scale exponent of an fp16 x 2 planes row (header: the row's largest magnitude lands in [2^14, 2^15)):
    e = exponent(max |y|) - 15 with max |y| = m 2^exponent, m in [0.5, 1); -15 for a zero row; clamped to [-100, 100]."""
    amax = y.abs().max(1).values
    e = torch.frexp(amax)[1].to(torch.int32) - 15
    return torch.where(amax > 0, e, torch.full_like(e, -15)).clamp(-100, 100)


def planes_view(buf, C, prow, fmt):
    """The packed-planes buffer as [C / 16 k-groups, prow / 32 row blocks, planes, 2 halves, 32 rows, 8 values] (header:
    1 KiB chunks per (k-group, 32-row block, plane))."""
    return buf.view(C // 16, prow // 32, 2 if fmt == "h2" else 3, 2, 32, 8)


# ------------------------------------------------------------------------------------------------ row softmax
def softmax_fwd_ref(s, cols, scale, keep_padding=False):
    """s [rows, ld] -> (p, bound) [rows, ld]: p[:, :cols] = softmax(scale s[:, :cols]) as exp(z - max z) / sum exp(z - max z),
    z = scale s (exact when scale = 1), p[:, cols:] = 0 exactly.  MUTATION keep_padding: the padding keeps its input."""
    sc = f32(scale)
    Z = _c(s[:, :cols])
    z = Z if sc == 1.0 else _rnd(Z[0] * sc, Z[1])
    zmax = z[0].max(1, keepdim=True).values
    m = (zmax, z[1].max(1, keepdim=True).values)          # |max z' - max z| <= max |z' - z|
    e = _exp(_sub(z, m))
    p = _mul(e, _recip(_sum(e, 1)), tiny=True)
    pad = s[:, cols:].double() if keep_padding else torch.zeros_like(s[:, cols:], dtype=torch.float64)
    return torch.cat((p[0], pad), 1), torch.cat((SECOND * p[1], torch.zeros_like(pad)), 1)


def softmax_bwd_ref(dp, p, cols, scale):
    """(ds, bound) [rows, ld]: ds = (scale p) (dp - sum_j dp_j p_j) on the GIVEN p (exact operand), 0 in the padding."""
    sc = f32(scale)
    D, P = _c(dp[:, :cols]), _c(p[:, :cols])
    t = _sub(D, _sum(_mul(D, P, tiny=True), 1))
    sp = P if sc == 1.0 else _rnd(P[0] * sc, P[1] + TINY)
    ds = _mul(sp, t, tiny=True)
    pad = torch.zeros_like(dp[:, cols:], dtype=torch.float64)
    return torch.cat((ds[0], pad), 1), torch.cat((SECOND * ds[1], pad), 1)


# ------------------------------------------------------------------------------------------------ L2 normalisation
def l2norm_fwd_ref(x, eps, clamp_squared=False):
    """x [rows, C] -> dict y / dy_ [rows, C], inv / dinv [rows]: inv = 1 / max(sqrt(sum x^2), eps), y = x inv (F.normalize).
    The clamp moves its operand's error at most one to one.  MUTATION clamp_squared: 1 / sqrt(max(sum x^2, eps))."""
    X = _c(x)
    q = _sum(_mul(X, X, tiny=True), 1)
    ev = torch.tensor(f32(eps), dtype=torch.float64, device=x.device)
    if clamp_squared:
        d = _sqrt((torch.maximum(q[0], ev), q[1]))
    else:
        s = _sqrt(q)
        d = (torch.maximum(s[0], ev), s[1])
    inv = _recip(d)
    y = _mul(X, inv)
    return dict(y=y[0], dy_=SECOND * y[1], inv=inv[0][:, 0], dinv=SECOND * inv[1][:, 0])


def l2norm_bwd_ref(dy, y, inv):
    """(dx, bound): dx = inv (dy - y <dy, y>) on the GIVEN y and inv (exact operands): the header's formula."""
    D, Y, I = _c(dy), _c(y), _c(inv[:, None])
    dx = _mul(I, _sub(D, _mul(Y, _sum(_mul(D, Y), 1))))
    return _out(dx)


# ------------------------------------------------------------------------------------------------ column sums
def colsum_ref(x, base=None, drop_row=None, twice_row=None):
    """(out, bound) [C]: out[c] = sum_r x[r, c] (+ base[c]); bound = (n + 8) U sum |x|, n the non-zero addends of the column
    (the header promises a fixed order, not which one), the accumulating addition one rounding more.  MUTATIONS: drop_row,
    twice_row (that row left out / counted twice)."""
    xd = x.double()
    w = torch.ones(x.shape[0], 1, dtype=torch.float64, device=x.device)
    if drop_row is not None:
        w[drop_row] = 0.0
    if twice_row is not None:
        w[twice_row] = 2.0
    n = (xd != 0).sum(0)
    assert int(n.max()) <= MAX_TERMS or bool((xd == xd.round()).all())
    out = ((xd * w).sum(0), (n + 8) * U * xd.abs().sum(0))
    if base is not None:
        out = _add(out, _c(base))
    return _out(out)


# ------------------------------------------------------------------------------------------------ exact movers
def chanmask_ref(x, mask, scale, rows_per_img):
    """out[r, c] = x[r, c] mask[r / rows_per_img, c] scale, fp32: exact for a 0 / 1 mask and a power-of-two scale."""
    img = torch.arange(x.shape[0], device=x.device) // rows_per_img
    return (x.double() * mask.double()[img] * scale).float()


def permute_rows_ref(x, outer, A, B, C):
    """[outer, A, B, C] -> [outer, B, A, C]"""
    return x.view(outer, A, B, C).permute(0, 2, 1, 3).reshape(outer * A * B, C)


def bound2_ref(rnorm, bias):
    return torch.stack((rnorm.max(), bias.abs().max() if bias is not None else torch.zeros((), device=rnorm.device)))


# ------------------------------------------------------------------------------------------------ shared inputs
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


LN_VARIANTS = ("n01", "bigmean", "outlier", "const", "tiny", "huge")
LN_CONST = 0.7                        # not dyadic: the fp32 sum of C copies need not be C times it
LN_EPS = (1e-6, 1e-5)
LN_FWD_C = (4, 12, 252, 256, 260, 768, 1024, 1028, 2052)    # C / 4: 1, 3, 63, 64, 65, 192, 256 (the last register-row width), 257, 513 (streaming)
LN_FWD_ROWS = (1, 3, 5, 33)
LN_FWD_BIG = (4 * 16384 + 5, 4)       # the second trip of the 16384-block grid of 4 rows
LN_PLANES_C = (16, 48, 768, 1040)
LN_PLANES_ROWS = (1, 31, 33, 65)
LN_PLANES_BIG = (32 * 16384 + 33, 16) # the same for the 32-row blocks of the plane-emitting forms
LN_BWD_C = (4, 12, 252, 256, 260, 768, 1024)
LN_BWD_ROWS = (1, 7, 9, 17)           # around the 8 rows of a block without weight-gradient partials
LN_BWD_ROWS_PARTS = (1, 63, 65, 129)  # around the 64 rows of a block with them
LN_BWD_BIG = (2048 * 64 + 67, 4)      # 2048 blocks of 65 rows (the last one shorter)
LN_BWD_BIG_LIVE = (0, 65 * 1000, 65 * 1000 + 64, 65 * 500 + 31, 2048 * 64 + 66)   # rows whose dy is not zero: first / last overall, first / last / middle of a block


def ln_parts_ref(rows):
    """svl_layernorm_bwd_parts of the header's geometry: ceil(rows / 64) blocks, 2048 at most."""
    return max(1, min(2048, (rows + 63) // 64))


def planes_rows_ref(rows):
    return (rows + 255) // 256 * 256


@functools.lru_cache(maxsize=4)
def ln_inputs(rows, C):
    """(x, dy, dx_add [rows, C], gamma, beta [C], eps) fp32 on the CPU, seeded by the shape.  Row i is of kind
    LN_VARIANTS[(i + k) % 6], k from the shape (so a one-row case is of a different kind at every C): N(0, 1); a mean of 100
    standard deviations; one outlier channel of 300 standard deviations; constant (variance 0); scaled by 1e-20 (variance far
    below eps); scaled by 1e15.  gamma around 1 (channel 2 negative), channel 1: gamma = beta = 0 (the exact zeros).  eps
    alternates between 1e-6 and 1e-5."""
    g = _gen(rows, C, 21)
    k = (C // 4 + rows) % len(LN_VARIANTS)
    x = torch.randn(rows, C, generator=g)
    kind = (torch.arange(rows) + k) % len(LN_VARIANTS)
    if (rows, C) == LN_BWD_BIG:       # N(0, 1) throughout: every live row weighs in dgamma
        kind = torch.zeros_like(kind)
    x[kind == 1] += 100.0
    out_rows = (kind == 2).nonzero()[:, 0]
    ch = torch.randint(0, C, (out_rows.numel(),), generator=g)
    x[out_rows, ch] += 300.0 * torch.where(torch.rand(out_rows.numel(), generator=g) < 0.5, -1.0, 1.0)
    x[kind == 3] = LN_CONST
    x[kind == 4] *= 1e-20
    x[kind == 5] *= 1e15
    dy, add = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    gamma[1], beta[1] = 0.0, 0.0
    gamma[2] = -gamma[2].abs()
    if (rows, C) == LN_BWD_BIG:
        live = torch.zeros(rows, 1)
        live[list(LN_BWD_BIG_LIVE)] = 1.0
        dy = dy * live
    return x, dy, add, gamma, beta, f32(LN_EPS[(C // 4 + rows) % 2])


SM_COLS = (1, 63, 64, 65, 1025)
SM_ROWS = (1, 5)
SM_SCALES = (1.0, 0.125)
SM_BIG = (4 * 65536 + 5, 3, 8)        # (rows, cols, ld): the second trip of the 65536-block grid of 4 rows


def sm_lds(cols):
    return (cols, cols + 3, (cols + 4) // 4 * 4 + 4)


@functools.lru_cache(maxsize=4)
def sm_inputs(rows, cols, ld, scale):
    """(s, dp [rows, ld]) fp32, finite; the padding [cols, ld) holds the sentinel.  Row i is of kind (i + k) % 4: N(0, 3);
    a spread of +-200; all equal (p = 1 / cols); one dominant entry."""
    g = _gen(rows, cols, ld, int(scale * 1000), 22)
    k = (cols + ld + int(scale * 8)) % 4
    kind = (torch.arange(rows) + k) % 4
    s = 3.0 * torch.randn(rows, ld, generator=g)
    s[kind == 1] = (400.0 * torch.rand(rows, ld, generator=g) - 200.0)[kind == 1]
    s[kind == 2] = 1.7
    dom = (kind == 3).nonzero()[:, 0]
    s[dom, torch.randint(0, cols, (dom.numel(),), generator=g)] += 60.0
    dp = torch.randn(rows, ld, generator=g)
    s[:, cols:], dp[:, cols:] = SENTINEL, SENTINEL
    return s, dp


L2_C = (1, 63, 64, 65, 512, 1000)
L2_ROWS = (1, 5)
L2_EPS = (0.0, 1e-12)
L2_BIG = (4 * 65536 + 3, 2)
L2_KINDS_CLAMP = ("n01", "zero", "norm1e-14", "small", "large")
L2_KINDS_OPEN = ("n01", "small", "large", "n01x3", "small")        # eps = 0: non-zero rows only


def l2_large(C):
    """Rows 'scaled by 1e18': the fp32 sum of C squares of that size passes FLT_MAX = 3.4e38 from C = 341 on (in the kernel
    as in any fp32 evaluation of the formula, F.normalize's included), so the wide rows are scaled by 1e17."""
    return 1e18 if C <= 128 else 1e17


@functools.lru_cache(maxsize=4)
def l2_inputs(rows, C, eps):
    """(x, dy [rows, C], kinds) fp32.  small / large: magnitudes in [0.5, 4.5] times 1e-18 / l2_large(C), so that every
    square is a normal number."""
    g = _gen(rows, C, int(eps > 0), 23)
    names = L2_KINDS_CLAMP if eps > 0 else L2_KINDS_OPEN
    kind = (torch.arange(rows) + C) % 5
    x = torch.randn(rows, C, generator=g)
    x = torch.where(x.abs() < 1e-3, torch.full_like(x, 0.5), x)        # (a one-channel row is not zero by chance)
    mag = (0.5 + torch.randn(rows, C, generator=g).abs().clamp_max(4.0)) * torch.where(torch.rand(rows, C, generator=g) < 0.5, -1.0, 1.0)
    for kd, nm in enumerate(names):
        sel = kind == kd
        if nm == "zero":
            x[sel] = 0.0
        elif nm == "norm1e-14":
            x[sel] = (x[sel].double() / x[sel].double().norm(dim=1, keepdim=True) * 1e-14).float()
        elif nm == "small":
            x[sel] = mag[sel] * 1e-18
        elif nm == "large":
            x[sel] = mag[sel] * l2_large(C)
        elif nm == "n01x3":
            x[sel] *= 3.0
    return x, torch.randn(rows, C, generator=g), [names[int(kd)] for kd in kind[:8]]


# (name, C, ld, off): off = the column of the wider matrix the operand starts at (off % 4 != 0: a pointer off 16-byte alignment)
CS_LAYOUTS = [
    ("scalar_c1", 1, 5, 4),
    ("scalar_c30", 30, 36, 4),
    ("scalar_ld_odd", 4, 10, 4),          # ld % 4 != 0
    ("scalar_ptr_off1", 8, 12, 1),        # x one float off alignment
    ("v4_c4", 4, 12, 4),                  # one column group, 256 row lanes
    ("v4_c12", 12, 20, 4),                # three of four groups live
    ("v4_c256", 256, 264, 4),             # 64 groups: exactly one block in x
    ("v4_c260", 260, 268, 4),             # the second block in x
]
CS_ROWS = (1, 255, 257, 1023, 1025)       # the unrolled-by-4 tails of 256 row lanes on both sides
CS_BIG = ("v4_chunk_cap", 1024 * 256 + 300, 4, 8, 4)     # 1024 chunks of 257 rows
CS_LONG = 65536                           # ops.colsum's reshaping route for one long column
CS_INT = 8                                # integer-valued data in [-8, 8]: |any partial sum| < 2^24, exact in every order


def cs_ints(rows, C, seed=0):
    return torch.randint(-CS_INT, CS_INT + 1, (rows, C), generator=_gen(rows, C, seed, 24)).float()


def cs_floats(rows, C):
    """(N(0, 1) data, a cancellation matrix: rows 2j and 2j + 1 hold +-v_j with |v_j| around 1e6, the last row (odd counts)
    or an added 2^-10 grid value the small remainder)."""
    g = _gen(rows, C, 25)
    a = torch.randn(rows, C, generator=g)
    v = 1e6 * (1.0 + torch.rand((rows + 1) // 2, C, generator=g))
    c = torch.stack((v, -v), 1).reshape(-1, C)[:rows].clone()
    rem = 0.01 * torch.randn(C, generator=g)
    c[-1] = (c[-1] + rem) if rows % 2 == 0 else rem
    return a, c[torch.randperm(rows, generator=g)]


PERMUTE_CASES = [(2, 3, 5, 4), (3, 7, 4, 260), (1, 5, 9, 4), (5, 81, 83, 4)]     # the last: 33615 rows > 4 * 8192 (the grid cap)
CHANMASK_CASES = [(37, 5, 7), (100, 9, 33), (1, 1, 1)]                            # (rows, rows_per_img, C): ragged last image, C odd
BOUND2_ROWS = (1, 255, 257)
