"""Plain float64 restatements of the channels-last image normalisations -- the GroupNorm family (svl_groupnorm_fwd / _apply /
_scale_shift / _bwd / _bwd_apply, csrc/norm.hip) and the BatchNorm chain (svl_bn_stats / _finalize / _eval_invstd / _apply /
_bwd_reduce / _bwd_apply, csrc/batchnorm.hip) -- each from the formulas of include/semivl_hip.h and the semantics of
torch.nn.functional.group_norm / batch_norm, none from the kernels.  Device-agnostic, like tests/spatial_ref.py, whose
strided / guard-band helpers and unit roundoff it reuses: tests/test_imgnorm_kernels_gpu.py runs them on the device,
tests/test_imgnorm_ref.py proves them on the CPU against ATen float64 and autograd.

Every restatement returns (want, bound).  `bound` is a FIRST-ORDER running error bound, element by element, of an fp32
evaluation of the header's formula (U = 2^-24 per rounded operation, Higham, Accuracy and Stability of Numerical Algorithms,
section 3.1): the error of an operand is carried through each operation with the operation's partial derivatives, and each
fp32 result adds U times its own magnitude.  Where the header leaves the association of a sum open (S1 + xhat S2), the
magnitude is taken as the sum of the magnitudes of its terms, which covers every association.  A statistic that the header
accumulates in double adds n 2^-53 sum |terms| for a sum of n terms.  Products of two error terms (second order) are
covered by the factor SECOND = 1 + 2^-10 on every bound: they are below 2^-10 of the first-order term while the relative
error of every intermediate is below 2^-10, which holds with a margin of 2^6 at the worst conditioned case here (a mean of
100 standard deviations: relative error of the centred value 100 U 2 = 2^-16).  No tolerance is chosen anywhere.

Outputs behind a fused ReLU: the pre-activation p carries the bound dp.  |p| > dp decides the mask for every evaluation
inside the bound: the output is then exactly 0 (bound 0: compared for equality) or p (bound dp).  An element with |p| <= dp
(and dp > 0) could fall on either side; the input builders below move such elements until NONE is left (`undecided` counts
them; tests/test_imgnorm_ref.py asserts the count is zero for every case), so the GPU file leaves no element out.  The
deliberately exact zeros (gamma = 0 and beta = 0: p = 0 with dp = 0) are masked on both sides and stay in.

Also here: the seeded case lists and input builders both test files share."""
import functools

import numpy as np
import torch

from spatial_ref import AGUARD, SENTINEL, U, gaps_intact, guard_intact, guarded, strided  # noqa: F401  (re-exported)

D = 2.0 ** -53                       # unit roundoff of float64
SECOND = 1.0 + 2.0 ** -10            # second-order terms, see the module docstring
EPS = float(np.float32(1e-5))        # eps is an fp32 argument of the C-ABI: the value the kernels see
GN_MAX_IMGS = 65535                  # images of an apply pass sit on gridDim.y
GN_WIDE = 262144                     # HW * C from which the statistics kernels run 1024 threads
GN_APPLY_CAP = 1024                  # blocks of PR * 8 pixels the apply passes launch at most
BN_GRID_CAP = 256 * 32               # blocks of 256 quads svl_bn_apply / _bwd_apply launch at most
BN_MAX_CHUNKS = 1024                 # row chunks of the two-stage BatchNorm reductions (256 rows each below the cap)


def f32(v):
    """The fp32 value of a Python float (momentum, eps: float arguments of the C-ABI)."""
    return float(np.float32(v))


def _per_channel(t, cg):
    """[imgs, G] -> [imgs, C]"""
    return t.repeat_interleave(cg, 1)


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_stats_ref(x, G, eps=EPS):
    """x [imgs, HW, C] -> dict of [imgs, G] float64: mean, rstd = 1 / sqrt(var + eps) (biased variance over the HW * C / G
    values of a group, F.group_norm) and their bounds dmean, drstd for the header's statistics: sums of x and x^2 in double,
    mean and rstd rounded to float.
      dmean = U |mean| + 2^-53 sum |x|                       (n 2^-53 sum |x| on the sum, divided by n)
      dvar  = (n + 8) 2^-53 (mean(x^2) + mean^2) + 2 |mean| 2^-53 sum |x|      (sum of squares, the square of the mean, their
                                                                                 difference; 8: the handful of double operations)
      drstd = rstd (U + dvar / (2 (var + eps)))              (d/dvar (var + eps)^-1/2 = -rstd / (2 (var + eps)))"""
    imgs, HW, C = x.shape
    cg = C // G
    n = HW * cg
    xg = x.double().view(imgs, HW, G, cg)
    m = xg.mean((1, 3))
    v = ((xg - m[:, None, :, None]) ** 2).mean((1, 3))
    r = 1.0 / torch.sqrt(v + eps)
    a1, a2 = xg.abs().sum((1, 3)), (xg * xg).sum((1, 3))
    dacc = D * a1
    dv = (n + 8) * D * (a2 / n + m * m) + 2 * m.abs() * dacc
    return dict(mean=m, rstd=r, var=v, dmean=SECOND * (U * m.abs() + dacc), drstd=SECOND * r * (U + dv / (2 * (v + eps))), G=G, cg=cg)


def gn_stats_pair(st):
    """([imgs, G, 2] (mean, rstd), bound) in the layout of the `stats` output."""
    return torch.stack((st["mean"], st["rstd"]), 2), torch.stack((st["dmean"], st["drstd"]), 2)


def gn_table_ref(st, gamma, beta):
    """The affine form of the header: y = fma(x, sc, sh), sc = rstd * gamma, sh = fma(-mean, sc, beta), per (image, channel).
    Returns (table [imgs, 2, C], bound): dsc = |gamma| drstd + U |sc|;  dsh = |sc| dmean + |mean| dsc + U |sh|."""
    cg = st["cg"]
    m, r, dm, dr = (_per_channel(st[k], cg) for k in ("mean", "rstd", "dmean", "drstd"))
    ga, be = gamma.double()[None, :], beta.double()[None, :]
    sc = r * ga
    dsc = SECOND * (ga.abs() * dr + U * sc.abs())
    sh = be - m * sc
    dsh = SECOND * (sc.abs() * dm + m.abs() * dsc + U * sh.abs())
    return torch.stack((sc, sh), 1), torch.stack((dsc, dsh), 1)


def gn_pre_ref(x, st, gamma, beta):
    """(p, dp): the pre-activation p = x sc + sh = (x - mean) rstd gamma + beta and dp = |x| dsc + dsh + U |p|."""
    t, dt = gn_table_ref(st, gamma, beta)
    xd = x.double()
    p = xd * t[:, 0][:, None, :] + t[:, 1][:, None, :]
    dp = SECOND * (xd.abs() * dt[:, 0][:, None, :] + dt[:, 1][:, None, :] + U * p.abs())
    return p, dp


def undecided(p, dp):
    """Elements whose ReLU mask an evaluation inside the bound could set either way."""
    return int(((p.abs() <= dp) & (dp > 0)).sum())


def relu_ref(p, dp):
    """(max(p, 0), bound) for decided pre-activations: exactly 0 behind the ReLU, dp in front of it."""
    on = p > 0
    return torch.where(on, p, torch.zeros_like(p)), torch.where(on, dp, torch.zeros_like(dp))


def gn_fwd_ref(x, gamma, beta, G, relu, eps=EPS):
    """dict: st (gn_stats_ref), y / dy_ (output and bound), p / dp (pre-activation), mask (p > 0, or all ones)."""
    st = gn_stats_ref(x, G, eps)
    p, dp = gn_pre_ref(x, st, gamma, beta)
    y, b = relu_ref(p, dp) if relu else (p, dp)
    return dict(st=st, y=y, bound=b, p=p, dp=dp, mask=(p > 0) if relu else torch.ones_like(p, dtype=torch.bool))


def gn_bwd_ref(x, dy, fwd, gamma, n_div=None, group_shift=0, drop_pixel=False):
    """GroupNorm (+ ReLU) backward in the header's form, from the forward's float64 statistics and mask:
      d' = dy masked;  A[img, c] = sum_p d',  B[img, c] = sum_p d' xhat,  xhat = (x - mean) rstd        (chan_sums, double sums
                                                                                                         rounded to float)
      S1 = sum_{c in group} gamma_c A_c,  S2 = sum_{c in group} gamma_c B_c                              (fp32, cg terms)
      dx = rstd (d' gamma - (S1 + xhat S2) / n),  n = HW cg;   dbeta = sum_img A,  dgamma = sum_img B    (fp32 column sums)
    Bounds, one rounding per product and sum:
      dxhat = rstd (dmean + U |x - mean|) + |x - mean| drstd + U |xhat|
      dA = HW 2^-53 sum |d'| + U |A|;   dB = sum |d'| dxhat + HW 2^-53 sum |d' xhat| + U |B|
      dS = sum |gamma| d(A or B) + cg U sum |gamma (A or B)|         (a product and at most cg - 1 additions per term)
      t1 = xhat S2: |S2| dxhat + |xhat| dS2 + U |t1|;   t2 = S1 + t1: dS1 + dt1 + U (|S1| + |t1|)
      t3 = t2 / n: (dt2 + 3 U (|S1| + |t1|)) / n        (fl(1 / fl(HW cg)): two roundings, the product: one)
      t5 = d' gamma - t3: U |d' gamma| + dt3 + U (|d' gamma| + (|S1| + |t1|) / n);   dx: |t5| drstd + rstd dt5 + U |dx|
      dbeta, dgamma: sum_img d(A, B) + (imgs + 8) U sum_img |A, B|   (no order of the column sum adds more than imgs + 8 terms in a chain)
    The keyword arguments are the seeded MUTATIONS of tests/test_imgnorm_ref.py: n_div (the divisor), group_shift (the
    statistics and sums of the neighbouring group), drop_pixel (the last pixel left out of A and B)."""
    st = fwd["st"]
    imgs, HW, C = x.shape
    cg, G = st["cg"], st["G"]
    n = float(HW * cg) if n_div is None else float(n_div)
    gsel = (torch.arange(G, device=x.device) + group_shift) % G
    m, r, dm, dr = (_per_channel(st[k][:, gsel], cg)[:, None, :] for k in ("mean", "rstd", "dmean", "drstd"))
    ga = gamma.double()
    d = dy.double() * fwd["mask"]
    xc = x.double() - m
    xh = xc * r
    dxh = r * (dm + U * xc.abs()) + xc.abs() * dr + U * xh.abs()
    ds, dsx, dsd = (d[:, :-1], (d * xh)[:, :-1], (d.abs() * dxh)[:, :-1]) if drop_pixel else (d, d * xh, d.abs() * dxh)
    A, B = ds.sum(1), dsx.sum(1)
    dA = HW * D * ds.abs().sum(1) + U * A.abs()
    dB = dsd.sum(1) + HW * D * dsx.abs().sum(1) + U * B.abs()

    def group(T, dT):
        gT = (ga * T).view(imgs, G, cg)
        S = gT.sum(2)
        dS = (ga.abs() * dT).view(imgs, G, cg).sum(2) + cg * U * gT.abs().sum(2)
        return _per_channel(S[:, gsel], cg)[:, None, :], _per_channel(dS[:, gsel], cg)[:, None, :]
    S1, dS1 = group(A, dA)
    S2, dS2 = group(B, dB)
    t1 = xh * S2
    dt1 = S2.abs() * dxh + xh.abs() * dS2 + U * t1.abs()
    mag = S1.abs() + t1.abs()
    dt3 = (dS1 + dt1 + U * mag + 3 * U * mag) / n
    t4 = d * ga
    t5 = t4 - (S1 + t1) / n
    dt5 = U * t4.abs() + dt3 + U * (t4.abs() + mag / n)
    dx = r * t5
    ddx = t5.abs() * dr + r * dt5 + U * dx.abs()
    k = (imgs + 8) * U
    return dict(dx=dx, ddx=SECOND * ddx, cs=torch.stack((A, B), 1), dcs=SECOND * torch.stack((dA, dB), 1),
                dbeta=A.sum(0), ddbeta=SECOND * (dA.sum(0) + k * A.abs().sum(0)),
                dgamma=B.sum(0), ddgamma=SECOND * (dB.sum(0) + k * B.abs().sum(0)))


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_stats_ref(x):
    """x [rows, C] -> (sums [2, C] = (sum x, sum x^2), bound = rows 2^-53 (sum |x|, sum x^2)): double accumulation."""
    xd = x.double()
    rows = xd.shape[0]
    s = torch.stack((xd.sum(0), (xd * xd).sum(0)))
    return s, SECOND * rows * D * torch.stack((xd.abs().sum(0), (xd * xd).sum(0)))


def bn_finalize_ref(sums, dsums, count, eps=EPS, momentum=0.1, running_mean=None, running_var=None, unbiased=True):
    """mean = sums0 / count, var = sums1 / count - mean^2 (biased, clamped at 0), invstd = 1 / sqrt(var + eps), rounded to
    float; running_mean <- (1 - momentum) running_mean + momentum mean, running_var the same with the UNBIASED variance
    var count / (count - 1) (var itself when count <= 1), like torch.  `dsums` is the bound of `sums` as an input.
      dmean = dsums0 / count + U |mean|
      dvar = dsums1 / count + 2 |mean| dsums0 / count + 8 2^-53 (sums1 / count + mean^2);  dinvstd = invstd (U + dvar / (2 (var + eps)))
      running: momentum d(mean or unbiased var) + U |new value|      (formed in double, rounded once)
    Returns dict of (want, bound) pairs: mean, invstd and, when given, running_mean, running_var."""
    count = float(count)
    mu = sums[0] / count
    ex2 = sums[1] / count
    var = (ex2 - mu * mu).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    dmu_in = dsums[0] / count
    dvar = dsums[1] / count + 2 * mu.abs() * dmu_in + 8 * D * (ex2 + mu * mu)
    out = dict(mean=(mu, SECOND * (dmu_in + U * mu.abs())), invstd=(inv, SECOND * inv * (U + dvar / (2 * (var + eps)))), var=var)
    if running_mean is not None:
        mom = f32(momentum)
        k = count / (count - 1.0) if (count > 1.0 and unbiased) else 1.0
        nrm = (1.0 - mom) * running_mean.double() + mom * mu
        nrv = (1.0 - mom) * running_var.double() + mom * var * k
        out["running_mean"] = (nrm, SECOND * (mom * dmu_in + U * nrm.abs()))
        out["running_var"] = (nrv, SECOND * (mom * k * dvar + U * nrv.abs()))
    return out


def bn_eval_invstd_ref(running_var, eps=EPS, eps_outside=False):
    """(1 / sqrt(running_var + eps), bound): three fp32 operations; the rounding of the sum passes the square root halved:
    2.5 U invstd.  eps_outside: the seeded mutation 1 / (sqrt(var) + eps)."""
    v = running_var.double()
    inv = 1.0 / (torch.sqrt(v) + eps) if eps_outside else 1.0 / torch.sqrt(v + eps)
    return inv, SECOND * 2.5 * U * inv


def bn_pre_ref(x, mean, dmean, invstd, dinvstd, gamma, beta, resid=None):
    """(p, dp, q): p = (x - mean) invstd gamma + beta [+ resid] (the header's expression, one rounding per operation), q the
    value before the residual.   t1 = x - mean: dmean + U |t1|;  t2 = t1 invstd: |invstd| dt1 + |t1| dinvstd + U |t2|;
    t3 = t2 gamma + beta: |gamma| dt2 + U |t2 gamma| + U |t3|;   + resid: U |p|."""
    ga, be = gamma.double(), beta.double()
    t1 = x.double() - mean
    dt1 = dmean + U * t1.abs()
    t2 = t1 * invstd
    dt2 = invstd.abs() * dt1 + t1.abs() * dinvstd + U * t2.abs()
    q = t2 * ga + be
    dq = ga.abs() * dt2 + U * (t2 * ga).abs() + U * q.abs()
    if resid is None:
        return q, SECOND * dq, q
    p = q + resid.double()
    return p, SECOND * (dq + U * p.abs()), q


def bn_bwd_ref(x, dy, mask, mean, dmean, invstd, dinvstd, gamma, count, rows_used=None):
    """BatchNorm (+ residual + ReLU) backward of the header:
      d' = dy masked (= dres, bit-defined);  sums0 = sum_r d',  sums1 = sum_r d' xhat,  xhat = (x - mean) invstd   (double sums)
      dx = gamma invstd (d' - sums0 / count - xhat sums1 / count);   dbeta = sums0, dgamma = sums1
    Bounds: dxhat = invstd (dmean + U |x - mean|) + |x - mean| dinvstd + U |xhat|
      dsums0 = rows 2^-53 sum |d'|;   dsums1 = sum |d'| dxhat + rows 2^-53 sum |d' xhat|
      s0, s1 rounded to float: + U |s|;  1 / count rounded: U;  t1 = xhat s1: |s1| dxhat + |xhat| ds1 + U |t1|;
      t2 = s0 + t1: ds0 + dt1 + U (|s0| + |t1|);  t3 = t2 / count: (dt2 + 2 U (|s0| + |t1|)) / count;
      t5 = d' - t3: dt3 + U (|d'| + (|s0| + |t1|) / count);  g = gamma invstd: |gamma| dinvstd + U |g|;  dx = g t5: |t5| dg + |g| dt5 + U |dx|
    Returns dict: dres, sums [2, C], dsums, dx, ddx.  rows_used (mutation): only that many rows enter the sums."""
    count = float(count)
    rows = x.shape[0]
    ga = gamma.double()
    d = dy.double() * mask
    xc = x.double() - mean
    xh = xc * invstd
    dxh = invstd * (dmean + U * xc.abs()) + xc.abs() * dinvstd + U * xh.abs()
    k = rows if rows_used is None else rows_used
    s0, s1 = d[:k].sum(0), (d * xh)[:k].sum(0)
    ds0 = rows * D * d[:k].abs().sum(0)
    ds1 = (d.abs() * dxh)[:k].sum(0) + rows * D * (d * xh)[:k].abs().sum(0)
    return dict(dres=d, sums=torch.stack((s0, s1)), dsums=SECOND * torch.stack((ds0, ds1)),
                **bn_dx_ref(d, xh, dxh, s0, ds0, s1, ds1, invstd, dinvstd, ga, count))


def bn_dx_ref(d, xh, dxh, s0, ds0, s1, ds1, invstd, dinvstd, ga, count):
    """The dx expression of bn_bwd_ref on given sums (the sums of all shards under SyncBN, count = all their rows)."""
    ds0 = ds0 + U * s0.abs()
    ds1 = ds1 + U * s1.abs()
    t1 = xh * s1
    dt1 = s1.abs() * dxh + xh.abs() * ds1 + U * t1.abs()
    mag = s0.abs() + t1.abs()
    dt3 = (ds0 + dt1 + U * mag + 2 * U * mag) / count
    t5 = d - (s0 + t1) / count
    dt5 = dt3 + U * (d.abs() + mag / count)
    g = ga * invstd
    dg = ga.abs() * dinvstd + U * g.abs()
    dx = g * t5
    return dict(dx=dx, ddx=SECOND * (t5.abs() * dg + g.abs() * dt5 + U * dx.abs()), xh=xh, dxh=dxh)


# ------------------------------------------------------------------------------------------------ shared inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(name, base):
    return base + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _affine_params(C, g):
    """gamma around 1 (channel 2 negative), beta of either sign with |beta| >= 0.05 (a constant image has the pre-activation
    beta: decided), channel 1 with gamma = beta = 0 (the exact zeros)."""
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = (0.05 + 0.1 * torch.randn(C, generator=g).abs()) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma[1], beta[1] = 0.0, 0.0
    gamma[2] = -gamma[2].abs()
    return gamma.float(), beta.float()


def _settle(t, pre, what):
    """Move the elements of `t` whose ReLU mask is not decided (with a margin of 2 on the bound) until none is left: each is
    stepped away from zero pre-activation by 2^-6 of its magnitude plus 2^-6.  pre(t) -> (p, dp).  The few moved elements
    change the statistics by far less than the margin, so one or two rounds settle."""
    for _ in range(8):
        p, dp = pre(t)
        bad = (p.abs() <= 2 * dp) & (dp > 0)
        if not bool(bad.any()):
            assert undecided(p, dp) == 0
            return t
        step = (t.abs() + 1.0) * 2.0 ** -6
        t = torch.where(bad, t + torch.where(torch.rand(t.shape, generator=_gen(int(bad.sum()))) < 0.5, -step, step), t)
    raise AssertionError(f"{what}: undecided ReLU masks remain")


# (name, imgs, HW, C, G, relu, variant).  PR = NT / (C / 4) pixel rows per trip of the statistics kernels, NT = 256 threads
# below HW * C = 262144 and 1024 from there on; the apply passes take 256 / (C / 4) * 8 pixels per block, 1024 blocks at most.
GN_CASES = [
    ("cq1_hw_below_pr", 3, 5, 4, 1, True, ""),                    # CQ = 1, PR = 256 > HW
    ("one_quad_per_group", 2, 77, 16, 4, True, ""),               # cg = 4
    ("c1024_g64_tail1", 2, 9, 1024, 64, True, ""),                # PR = 1, G = 64, the 4x loop twice plus a tail of 1
    ("hw1", 1, 1, 256, 64, False, ""),                            # HW = 1
    ("tail_4pr_plus_1", 2, 65, 64, 4, True, ""),                  # PR = 16: 4 PR + 1
    ("tail_4pr_minus_1", 2, 63, 64, 4, False, ""),                # 4 PR - 1
    ("tail_2pr_plus_1", 2, 33, 64, 4, True, ""),                  # 2 PR + 1
    ("wide_at_switch", 1, 4096, 64, 4, True, ""),                 # HW * C = 262144: 1024 threads
    ("narrow_below_switch", 1, 4095, 64, 4, True, ""),            # the same data minus a pixel: 256 threads
    ("wide_pr4", 1, 256, 1024, 64, True, ""),                     # NT = 1024 with PR = 4
    ("apply_second_trip", 1, 8269, 1024, 64, True, ""),           # 8269 > 1024 blocks * 8 pixels: second trip of the apply grid
    ("cg512", 2, 30 * 23, 512, 1, True, ""),                      # cg = 512 terms in S1 / S2
    ("one_quad_per_group_bigmean", 2, 77, 16, 4, True, "bigmean"),
    ("one_quad_per_group_const", 2, 77, 16, 4, True, "const"),
    ("tail_4pr_plus_1_bigmean", 2, 65, 64, 4, True, "bigmean"),
    ("tail_4pr_plus_1_const", 2, 65, 64, 4, False, "const"),
]
GN_CONST = 3.0


def gn_case(name):
    return next(c for c in GN_CASES if c[0] == name)


@functools.lru_cache(maxsize=3)
def gn_inputs(case):
    """(x [imgs, HW, C], dy like x, gamma [C], beta [C]) fp32 on the CPU, seeded by the case's name; the two switch cases share
    their data.  variant bigmean: a mean of 100 standard deviations; const: every value 3.0 (variance exactly 0)."""
    name, imgs, HW, C, G, relu, variant = case
    if name == "narrow_below_switch":
        x, dy, gamma, beta = gn_inputs(gn_case("wide_at_switch"))
        x, dy = x[:, :HW].contiguous(), dy[:, :HW].contiguous()
    else:
        g = _gen(_seed(name, 11000))
        x = torch.randn(imgs, HW, C, generator=g) + 0.25
        dy = torch.randn(imgs, HW, C, generator=g)
        gamma, beta = _affine_params(C, g)
        if variant == "bigmean":
            x = x + 100.0
        elif variant == "const":
            x = torch.full_like(x, GN_CONST)
    if relu and variant != "const":
        x = _settle(x, lambda t: gn_pre_ref(t, gn_stats_ref(t, G), gamma, beta), name)
    return x, dy, gamma, beta


# (name, rows, C, relu, res, variant, momentum, running).  Stage 1 of the reductions takes min(1024, ceil(rows / 256)) row
# chunks; stage 2's 8-way unrolled loop is entered by chunk lane ky when chunks > 28 + ky; the elementwise passes launch at
# most 8192 blocks of 256 channel quads.
BN_CASES = [
    ("count1", 1, 4, False, False, "", 0.1, True),                # count = 1: the unbiased-variance guard
    ("idle_lanes_c12", 5, 12, True, False, "", 1.0, True),        # cgp = 4 > C / 4 = 3
    ("idle_lanes_c20", 300, 20, True, False, "", 0.1, True),      # cgp = 8 > 5
    ("two_col_blocks_c260", 513, 260, True, False, "", 0.1, False),   # 65 quads: two column blocks, 63 idle lanes; no running stats
    ("stage2_some_lanes", 256 * 29 + 3, 8, True, False, "", 0.1, True),   # 30 chunks: lanes ky = 0, 1 enter the unrolled loop
    ("stage2_loop_and_tail", 256 * 61 + 1, 8, False, False, "", 1.0, True),  # 62 chunks: the unrolled loop, then a tail
    ("chunk_cap", 262144 + 257, 4, True, False, "", 0.1, True),   # 1024 chunks of 257 rows
    ("grid_second_trip", 262401, 32, True, False, "", 0.1, True), # 262401 * 8 quads > 8192 * 256
    ("resid_relu", 646, 256, True, True, "", 0.1, True),          # residual + ReLU, every ld distinct
    ("idle_lanes_c20_bigmean", 300, 20, True, False, "bigmean", 0.1, True),
    ("resid_relu_bigmean", 646, 256, True, True, "bigmean", 1.0, True),
]
BN_CONST = -1.5
BN_SHARD = ("idle_lanes_c20", 130)                                # the SyncBN case: this batch as shards of 130 and 170 rows


def bn_case(name):
    return next(c for c in BN_CASES if c[0] == name)


def bn_fwd_from_x(x, gamma, beta, resid, relu, momentum=0.1, rm=None, rv=None, count=None):
    """The forward chain in float64 from x alone: dict sums / dsums, fin (bn_finalize_ref), p / dp, y / bound, mask."""
    sums, dsums = bn_stats_ref(x)
    fin = bn_finalize_ref(sums, dsums, x.shape[0] if count is None else count, EPS, momentum, rm, rv)
    p, dp, q = bn_pre_ref(x, *fin["mean"], *fin["invstd"], gamma, beta, resid)
    y, b = relu_ref(p, dp) if relu else (p, dp)
    return dict(sums=sums, dsums=dsums, fin=fin, p=p, dp=dp, q=q, y=y, bound=b,
                mask=(p > 0) if relu else torch.ones_like(p, dtype=torch.bool))


@functools.lru_cache(maxsize=3)
def bn_inputs(case):
    """(x [rows, C], dy, gamma, beta, resid or None, running_mean, running_var) fp32 on the CPU.  Channel 1: gamma = beta = 0;
    channel 3 (C >= 4, rows > 1): the constant dyadic value -1.5; variant bigmean: a mean of 100 standard deviations."""
    name, rows, C, relu, res, variant, momentum, running = case
    g = _gen(_seed(name, 12000))
    x = 2.0 * torch.randn(rows, C, generator=g) + 0.5
    dy = torch.randn(rows, C, generator=g)
    gamma, beta = _affine_params(C, g)
    resid = torch.randn(rows, C, generator=g) if res else None
    rm, rv = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    if variant == "bigmean":
        x = x + 200.0
    if rows > 1:
        x[:, 3] = BN_CONST
    if relu and res:
        resid = _settle(resid, lambda t: _pd(bn_fwd_from_x(x, gamma, beta, t, True)), name)
    elif relu:
        keep = x[:, 3].clone()
        x = _settle(x, lambda t: _pd(bn_fwd_from_x(t, gamma, beta, None, True)), name)
        assert torch.equal(x[:, 3], keep) or rows == 1, name       # the constant channel is decided by |beta| >= 0.05
    return x, dy, gamma, beta, resid, rm, rv


def _pd(f):
    return f["p"], f["dp"]
