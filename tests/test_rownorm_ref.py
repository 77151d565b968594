"""CPU: the restatements of tests/rownorm_ref.py proved against independent expressions (ATen float64 F.layer_norm / softmax /
F.normalize and their autograd), the derived bounds measured on the very inputs tests/test_rownorm_kernels_gpu.py uses (a plain
fp32 evaluation of the header's formulas, in torch on the CPU, has to stay inside each of them: the condition that the bounds
are honest, from the reference alone), and the evidence that the bounds would catch a subtly wrong kernel: eleven seeded
mutations, each of which has to leave the bound on at least one case.  -s prints the worst measured-to-bound ratio per entry
point."""
import collections
import itertools

import pytest
import torch
import torch.nn.functional as F

import rownorm_ref as R

TIGHT = 1e-9          # float64 restatement against float64 ATen, relative to the largest magnitude of each row (conditioning <= 1e5)
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"[largest fp32 error / bound] {k}: {WORST[k]:.3f}")


def _close(a, b, tol=TIGHT):
    if a.numel() == 0:
        return a.shape == b.shape
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    return bool(((a - b).abs().max(1).values <= tol * b.abs().max(1).values + 1e-30).all())


def _ratio(entry, tag, got, want, bound):
    """max |got - want| / bound; where the bound is zero the values have to be equal."""
    err = (got.double() - want).abs()
    z = bound <= 0
    assert bool((err[z] == 0).all()), (entry, tag)
    r = float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0
    WORST[entry] = max(WORST[entry], r)
    assert r <= 1.0, (entry, tag, r)
    return r


def _exceeds(mut, want, bound):
    """Some element is NOT inside the bound (a NaN is outside)."""
    return not bool(((mut.double() - want).abs() <= bound).all())


def _ln_shapes(Cs, rows, big=None):
    return [(r, C) for C in Cs for r in rows] + ([big] if big else [])


LN_FWD = _ln_shapes(R.LN_FWD_C, R.LN_FWD_ROWS, R.LN_FWD_BIG) + _ln_shapes(R.LN_PLANES_C, R.LN_PLANES_ROWS)
LN_BWD = _ln_shapes(R.LN_BWD_C, R.LN_BWD_ROWS + R.LN_BWD_ROWS_PARTS[1:], R.LN_BWD_BIG)
SM = [(r, c, ld, sc) for c in R.SM_COLS for ld in R.sm_lds(c) for r in R.SM_ROWS for sc in R.SM_SCALES] + [R.SM_BIG + (0.125,)]
L2 = [(r, C, e) for C in R.L2_C for r in R.L2_ROWS for e in R.L2_EPS] + [R.L2_BIG + (1e-12,), R.L2_BIG + (0.0,)]
CS = [(C, r) for _, C, _, _ in R.CS_LAYOUTS for r in R.CS_ROWS]


# ------------------------------------------------------------------------------------------------ plain fp32 evaluations
def _ln_fwd_fp32(x, gamma, beta, eps):
    C = x.shape[1]
    mean = x.sum(1, keepdim=True) / C
    a = x - mean
    rstd = 1.0 / torch.sqrt((a * a).sum(1, keepdim=True) / C + eps)
    return a * rstd * gamma + beta, torch.cat((mean, rstd), 1)


def _ln_bwd_fp32(dy, x, stats, gamma, add):
    C = x.shape[1]
    mean, rstd = stats[:, 0:1], stats[:, 1:2]
    xh = (x - mean) * rstd
    g = dy * gamma
    m1, m2 = g.sum(1, keepdim=True) / C, (g * xh).sum(1, keepdim=True) / C
    dx = rstd * (g - m1 - xh * m2)
    return (dx + add if add is not None else dx), (dy * xh).sum(0), dy.sum(0)


def _softmax_fwd_fp32(s, cols, scale, max_unscaled=False):
    z = s[:, :cols] * scale
    m = (s[:, :cols] if max_unscaled else z).max(1, keepdim=True).values
    e = torch.exp(z - m)
    return torch.cat((e * (1.0 / e.sum(1, keepdim=True)), torch.zeros_like(s[:, cols:])), 1)


def _softmax_bwd_fp32(dp, p, cols, scale):
    d, q = dp[:, :cols], p[:, :cols]
    return torch.cat((scale * q * (d - (d * q).sum(1, keepdim=True)), torch.zeros_like(dp[:, cols:])), 1)


def _l2_fwd_fp32(x, eps):
    inv = 1.0 / torch.sqrt((x * x).sum(1, keepdim=True)).clamp_min(eps)
    return x * inv, inv[:, 0]


def _l2_bwd_fp32(dy, y, inv):
    return inv[:, None] * (dy - y * (dy * y).sum(1, keepdim=True))


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("shape", LN_FWD + [R.LN_PLANES_BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_layernorm_fwd_restatement_and_bound(shape):
    x, dy, add, gamma, beta, eps = R.ln_inputs(*shape)
    C = shape[1]
    w = R.ln_fwd_ref(x, gamma, beta, eps)
    xd = x.double()
    assert _close(w["y"], F.layer_norm(xd, (C,), gamma.double(), beta.double(), eps))
    assert _close(w["stats"][:, :1], xd.mean(1, keepdim=True))
    assert _close(w["stats"][:, 1:], 1 / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps), 1e-7)
    y, st = _ln_fwd_fp32(x, gamma, beta, eps)
    _ratio("svl_layernorm_fwd", f"y {shape}", y, w["y"], w["dy_"])
    _ratio("svl_layernorm_fwd", f"stats {shape}", st, w["stats"], w["dstats"])
    assert bool((w["dy_"][:, 1] == 0).all()) and bool((w["y"][:, 1] == 0).all())        # gamma = beta = 0: exact zeros
    assert bool((w["dy_"][:, 0] > 0).all())


@pytest.mark.parametrize("shape", LN_BWD, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layernorm_bwd_restatement_and_bound(shape):
    x, dy, add, gamma, beta, eps = R.ln_inputs(*shape)
    C = shape[1]
    # the restatement on exact statistics is autograd of F.layer_norm
    w = R.ln_fwd_ref(x, gamma, beta, eps)
    xd, ga, be = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    gx, gg, gb = torch.autograd.grad(F.layer_norm(xd, (C,), ga, be, eps), (xd, ga, be), dy.double())
    b = R.ln_bwd_ref(dy, x, w["stats"], gamma, add)
    assert _close(b["dx"], gx + add.double(), 1e-7)
    assert _close(b["dgamma"][None], gg[None], 1e-7) and _close(b["dbeta"][None], gb[None])
    # a plain fp32 evaluation on fp32 statistics stays inside the bounds, with and without dx_add
    _, st = _ln_fwd_fp32(x, gamma, beta, eps)
    for a in (add, None):
        b = R.ln_bwd_ref(dy, x, st, gamma, a)
        dx, dg, db = _ln_bwd_fp32(dy, x, st, gamma, a)
        _ratio("svl_layernorm_bwd", f"dx {shape}", dx, b["dx"], b["ddx"])
    _ratio("svl_layernorm_bwd", f"dgamma {shape}", dg, b["dgamma"], b["ddgamma"])
    _ratio("svl_layernorm_bwd", f"dbeta {shape}", db, b["dbeta"], b["ddbeta"])


def test_layernorm_big_backward_case_is_sparse_and_sharp():
    """rows = 2048 * 64 + 67: 65 rows per block.  dy lives in five rows (first / last overall, first / last / middle of a
    block), so dgamma / dbeta have five addends and a tight bound: a dropped row leaves it by a factor above 10."""
    rows, C = R.LN_BWD_BIG
    assert (rows + R.ln_parts_ref(rows) - 1) // R.ln_parts_ref(rows) == 65 and R.ln_parts_ref(rows) == 2048
    x, dy, add, gamma, beta, eps = R.ln_inputs(rows, C)
    live = sorted(R.LN_BWD_BIG_LIVE)
    assert (dy != 0).any(1).nonzero()[:, 0].tolist() == live
    assert {r % 65 for r in live} >= {0, 64, 31} and live[0] == 0 and live[-1] == rows - 1
    _, st = _ln_fwd_fp32(x, gamma, beta, eps)
    b = R.ln_bwd_ref(dy, x, st, gamma)
    assert bool((b["ddx"][(dy == 0).all(1)] == 0).all())           # dx of a row without dy: exactly zero
    for r in live:
        m = R.ln_bwd_ref(dy, x, st, gamma, drop_row=r)
        for k in ("dgamma", "dbeta"):
            factor = ((m[k] - b[k]).abs() / b["d" + k]).max()
            assert float(factor) > 10.0, (r, k, float(factor))


def _exceeding(shapes, mutate):
    """(first shape at which the mutation leaves a bound, how many of the shapes it leaves one at, their number)."""
    hits = [shape for shape in shapes if mutate(shape)]
    return (hits[0] if hits else None), len(hits), len(shapes)


def test_layernorm_mutations_leave_the_bounds():
    small = [s for s in LN_FWD if s[0] <= 65]

    def fwd(**kw):
        def mutate(shape):
            x, dy, add, gamma, beta, eps = R.ln_inputs(*shape)
            w, m = R.ln_fwd_ref(x, gamma, beta, eps), R.ln_fwd_ref(x, gamma, beta, eps, **kw)
            return _exceeds(m["y"], w["y"], w["dy_"]) and _exceeds(m["stats"], w["stats"], w["dstats"])
        return mutate

    def bwd(which):
        def mutate(shape):
            x, dy, add, gamma, beta, eps = R.ln_inputs(*shape)
            _, st = _ln_fwd_fp32(x, gamma, beta, eps)
            w = R.ln_bwd_ref(dy, x, st, gamma, add)
            if which == "m2":
                return _exceeds(R.ln_bwd_ref(dy, x, st, gamma, add, drop_m2=True)["dx"], w["dx"], w["ddx"])
            if which == "add":
                return _exceeds(R.ln_bwd_ref(dy, x, st, gamma, None)["dx"], w["dx"], w["ddx"])
            m = R.ln_bwd_ref(dy, x, st, gamma, add, drop_row=shape[0] - 1)
            return _exceeds(m["dgamma"], w["dgamma"], w["ddgamma"]) and _exceeds(m["dbeta"], w["dbeta"], w["ddbeta"])
        return mutate

    bsmall = [s for s in LN_BWD if s[0] <= 129]
    for name, (hit, n, of) in (("divisor C - 1", _exceeding(small, lambda s: fwd(divisor=s[1] - 1)(s))),
                      ("sqrt(var) + eps", _exceeding(small, fwd(eps_outside=True))),
                      ("last quad left out of the mean", _exceeding([s for s in small if s[1] > 4], fwd(mean_drops_quad=True))),
                      ("m2 term dropped", _exceeding(bsmall, bwd("m2"))),
                      ("dx_add dropped", _exceeding(bsmall, bwd("add"))),
                      ("row dropped from dgamma / dbeta", _exceeding(bsmall, bwd("row")))):
        print(f"[mutation] {name}: outside the bound at {n} of {of} shapes, first at rows x C = {hit}")
        assert hit is not None, name


# ------------------------------------------------------------------------------------------------ row softmax
@pytest.mark.parametrize("case", SM, ids=lambda c: "-".join(map(str, c)))
def test_softmax_rows_restatement_and_bound(case):
    rows, cols, ld, scale = case
    s, dp = R.sm_inputs(*case)
    w, bw = R.softmax_fwd_ref(s, cols, scale)
    sd = (s.double()[:, :cols] * scale).requires_grad_(True)
    p64 = torch.softmax(sd, 1)
    assert _close(w[:, :cols], p64.detach()) and bool((w[:, cols:] == 0).all()) and bool((bw[:, cols:] == 0).all())
    p = _softmax_fwd_fp32(s, cols, scale)
    _ratio("svl_softmax_rows_fwd", f"{case}", p, w, bw)
    assert abs(float((p.double().sum(1) - 1).abs().max())) <= float(bw.sum(1).max())
    # backward on the exact p is autograd; on the fp32 p it is held to its bound
    g, _ = R.softmax_bwd_ref(dp, torch.cat((p64.detach(), w[:, cols:]), 1), cols, scale)
    assert _close(g[:, :cols], torch.autograd.grad(p64, sd, dp.double()[:, :cols])[0] * scale, 1e-7)
    g, bg = R.softmax_bwd_ref(dp, p, cols, scale)
    _ratio("svl_softmax_rows_bwd", f"{case}", _softmax_bwd_fp32(dp, p, cols, scale), g, bg)
    assert bool((bg[:, cols:] == 0).all())


def test_softmax_mutations_leave_the_bounds():
    """The padding left as it was: caught in float64.  The scale applied after the maximum was taken of the UNSCALED row:
    in exact arithmetic exp(scale s - max s) / sum(...) is the same function for scale > 0 (the constant cancels), so a
    float64 mutation cannot leave any bound; what such a kernel gets wrong is the range of fp32 -- on the +-200 rows with
    scale 0.125 every exponent is below -174, every expf is 0 and the row is 0 / 0 (a negative row overflows instead: inf /
    inf).  The mutation is therefore evaluated in fp32, as the kernel would."""
    pad = scaled = None
    for case in SM[:-1]:
        rows, cols, ld, scale = case
        s, dp = R.sm_inputs(*case)
        w, bw = R.softmax_fwd_ref(s, cols, scale)
        if ld > cols and _exceeds(R.softmax_fwd_ref(s, cols, scale, keep_padding=True)[0], w, bw):
            pad = pad or case
        if scale != 1.0 and _exceeds(_softmax_fwd_fp32(s, cols, scale, max_unscaled=True), w, bw):
            scaled = scaled or case
            assert not _exceeds(_softmax_fwd_fp32(s, cols, scale), w, bw)
    print(f"[mutation] padding not zeroed: outside the bound at {pad}; scale after the max subtraction only: at {scaled}")
    assert pad is not None and scaled is not None


# ------------------------------------------------------------------------------------------------ L2 normalisation
@pytest.mark.parametrize("case", L2, ids=lambda c: "-".join(map(str, c)))
def test_l2norm_restatement_and_bound(case):
    rows, C, eps = case
    x, dy, kinds = R.l2_inputs(*case)
    e32 = R.f32(eps)
    w = R.l2norm_fwd_ref(x, eps)
    xd = x.double().requires_grad_(True)
    y64 = F.normalize(xd, dim=1, eps=e32) if eps > 0 else xd / xd.norm(dim=1, keepdim=True)
    assert _close(w["y"], y64.detach())
    nrm = x.double().norm(dim=1)
    clamped = nrm < e32
    if eps > 0:         # the landmarks: a zero row and a row of norm 1e-14 give y = x / eps and inv = 1 / eps
        assert bool((w["inv"][clamped] == 1.0 / e32).all())
        assert not bool(clamped.any()) or _close(w["y"][clamped], x.double()[clamped] / e32, 1e-15)
        assert {"zero", "norm1e-14"} <= set(R.L2_KINDS_CLAMP) and (rows < 5 or int(clamped.sum()) >= 3 * (rows // 5))
    else:
        assert bool((nrm > 0).all())
    y, inv = _l2_fwd_fp32(x, e32)
    _ratio("svl_l2norm_fwd", f"y {case}", y, w["y"], w["dy_"])
    _ratio("svl_l2norm_fwd", f"inv {case}", inv, w["inv"], w["dinv"])
    # backward: the header's formula is autograd while the clamp is inactive
    g, _ = R.l2norm_bwd_ref(dy, w["y"], w["inv"])
    gx = torch.autograd.grad(y64, xd, dy.double())[0]
    scale = w["inv"] * dy.double().abs().max(1).values          # (one channel: the gradient is 0 = inv (dy - dy), cancelled at this scale)
    assert bool((((g - gx).abs().max(1).values <= 1e-7 * scale) | clamped).all())
    g, bg = R.l2norm_bwd_ref(dy, y, inv)
    _ratio("svl_l2norm_bwd", f"{case}", _l2_bwd_fp32(dy, y, inv), g, bg)


def test_l2norm_clamp_mutation_leaves_the_bound():
    hit = None
    for case in L2[:-2]:
        if case[2] > 0:
            x, dy, _ = R.l2_inputs(*case)
            w, m = R.l2norm_fwd_ref(x, case[2]), R.l2norm_fwd_ref(x, case[2], clamp_squared=True)
            if _exceeds(m["inv"], w["inv"], w["dinv"]) and _exceeds(m["y"], w["y"], w["dy_"]):
                hit = hit or case
    print(f"[mutation] clamp max(norm^2, eps): outside the bound at {hit}")
    assert hit is not None


def test_l2norm_bwd_formula_against_autograd_under_the_clamp():
    """Where the clamp is active (||x|| < eps) y = x / eps and the gradient is dy / eps; the header's formula gives
    (dy - y <dy, y>) / eps: the two differ by y <dy, y> / eps, relative to dy / eps by up to |y|^2 = (||x|| / eps)^2 -- 1e-4 for
    the row of norm 1e-14 under eps = 1e-12 -- and agree for a zero row (y = 0).  The project calls the kernel with eps in
    {0, 1e-12} on CLIP embeddings (norms of order 1 to 10): the sentence in the header is the outcome, the kernel stays."""
    eps = R.f32(1e-12)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 64, generator=g).double()
    x[0] = 0.0
    x[1] = x[1] / x[1].norm() * 1e-14
    x[2] = x[2] / x[2].norm() * 0.5e-12
    dy = torch.randn(3, 64, generator=g).double()
    xd = x.clone().requires_grad_(True)
    y = F.normalize(xd, dim=1, eps=eps)
    gx = torch.autograd.grad(y, xd, dy)[0]
    assert _close(gx, dy / eps)
    inv = torch.full((3,), 1.0 / eps, dtype=torch.float64)
    hdr = inv[:, None] * (dy - y.detach() * (dy * y.detach()).sum(1, keepdim=True))
    assert _close(hdr[:1], gx[:1], 1e-15)                               # the zero row: the same, to the rounding of float64
    gap = (hdr - gx).abs().max(1).values / gx.abs().max(1).values
    print(f"[l2norm_bwd under the clamp] relative gap to autograd: zero row {float(gap[0]):.1e}, norm 1e-14 {float(gap[1]):.1e}, "
          f"norm eps / 2 {float(gap[2]):.1e}")
    assert _close(hdr, gx - y.detach() * (dy * y.detach()).sum(1, keepdim=True) / eps, 1e-14)
    assert 0 < float(gap[1]) <= 1e-4 and 0.01 < float(gap[2]) <= 0.25


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("case", CS, ids=lambda c: f"{c[1]}x{c[0]}")
def test_colsum_restatement_and_bound(case):
    C, rows = case
    a, c = R.cs_floats(rows, C)
    base = torch.randn(C, generator=torch.Generator().manual_seed(rows + C))
    for x in (a, c):
        w, bw = R.colsum_ref(x)
        assert _close(w[None], x.double().sum(0)[None])
        _ratio("svl_colsum_f32", f"{case}", x.sum(0), w, bw)
        w, bw = R.colsum_ref(x, base=base)
        _ratio("svl_colsum_f32", f"accumulate {case}", base + x.sum(0), w, bw)
    xi = R.cs_ints(rows, C)
    w, _ = R.colsum_ref(xi)
    assert torch.equal(w, w.round()) and float(xi.abs().sum(0).max()) < 2 ** 24 and torch.equal(xi.sum(0).double(), w)


def test_colsum_mutations_leave_the_bounds():
    dropped = twice = None
    for C, rows in CS:
        a, _ = R.cs_floats(rows, C)
        xi = R.cs_ints(rows, C)
        r = rows // 2
        w, bw = R.colsum_ref(a)
        wi, _ = R.colsum_ref(xi)
        if bool((xi[r] != 0).any()):
            assert not torch.equal(R.colsum_ref(xi, drop_row=r)[0], wi) and not torch.equal(R.colsum_ref(xi, twice_row=r)[0], wi)
        if _exceeds(R.colsum_ref(a, drop_row=r)[0], w, bw):
            dropped = dropped or (C, rows)
        if _exceeds(R.colsum_ref(a, twice_row=r)[0], w, bw):
            twice = twice or (C, rows)
    big = R.cs_ints(R.CS_BIG[1], R.CS_BIG[2])
    assert float(big.abs().sum(0).max()) < 2 ** 24
    print(f"[mutation] row dropped from a column sum: outside the bound at (C, rows) = {dropped}; row counted twice: at {twice}")
    assert dropped is not None and twice is not None


# ------------------------------------------------------------------------------------------------ movers and landmarks
def test_movers_and_exponents():
    x = torch.arange(2 * 3 * 5 * 4, dtype=torch.float32).view(-1, 4)
    p = R.permute_rows_ref(x, 2, 3, 5, 4).view(2, 5, 3, 4)
    assert all(torch.equal(p[o, b, a], x.view(2, 3, 5, 4)[o, a, b]) for o, a, b in itertools.product(range(2), range(3), range(5)))
    y = torch.tensor([[0.0, 0.0], [1.0, -0.5], [2.0 ** 14, 1.0], [0.75 * 2.0 ** -20, 0.0], [3e38, 0.0], [1e-45, 0.0]])
    assert R.sexp_ref(y).tolist() == [-15, -14, 0, -35, 100, -100]
    e = R.sexp_ref(y[1:5]).double()
    scaled = y[1:5].abs().max(1).values.double() * 2.0 ** -e
    assert bool(((scaled >= 2 ** 14) & (scaled < 2 ** 15))[:3].all())
    m = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    xx = torch.randn(5, 3, generator=torch.Generator().manual_seed(3))
    assert torch.equal(R.chanmask_ref(xx, m, 2.0, 3), xx * m[[0, 0, 0, 1, 1]] * 2.0)
    assert R.bound2_ref(torch.tensor([1.0, 3.0, 2.0]), torch.tensor([-4.0, 1.0])).tolist() == [3.0, 4.0]
    assert R.ln_parts_ref(1) == 1 and R.ln_parts_ref(65) == 2 and R.planes_rows_ref(257) == 512
