"""GPU: the row half of csrc/norm.hip -- LayerNorm (svl_layernorm_fwd / _fwd_planes / _fwd_planes_f16x2 / _bwd in its four
forms), svl_softmax_rows_fwd / _bwd, svl_l2norm_fwd / _bwd, svl_colsum_f32 (both stage-1 kernels, accumulate 0 and 1, the
ops.colsum route for one long column) and the exact movers svl_chanmask_f32 / svl_permute_rows_f32 / svl_bound2_f32 -- against
the float64 restatements of tests/rownorm_ref.py under the bounds derived there: no tolerance is chosen here.

Every output goes into a sentinel-filled buffer with guard bands that must come back intact; the strided operand of the
column sums is a column slice at a non-zero offset of a wider sentinel matrix, which must not change (a softmax matrix is
written over its whole stride: its padding must come back as exact zeros, its guard bands intact); everything runs twice for a
bit-for-bit comparison; -s prints max error / bound, which has to be <= 1.  No element is left out of any comparison; exact
zeros (gamma = beta = 0, dx where dy = 0, softmax padding, the y of a zero row) and integer-valued column sums are compared
for equality.

The shapes reach what the N(0, 1), C in {256, 768, 1024} cases of tests/test_ops_gpu.py do not: C / 4 below 64 and off its
multiples, the last register-row width and the streaming branch, the second trip of every capped grid, more than 64 rows per
block of the weight-gradient partials, rows with a large mean, an outlier channel, zero variance and extreme scales, the
clamp of the L2 normalisation, every stage-1 kernel choice of the column sums with both tails of its unrolled loop, and
every argument refusal."""
import collections
import re

import pytest
import torch

import rownorm_ref as R

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(float)     # entry point -> largest error / bound of the session (printed at the end under -s)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"[largest error / bound] {k}: {WORST[k]:.3f}")


def _ratio(entry, tag, got, want, bound):
    """max |got - want| / bound; where the bound is zero the result has to be equal."""
    err = (got.double() - want).abs()
    z = bound <= 0
    assert bool((err[z] == 0).all()), (entry, tag)
    r = float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0
    print(f"[{entry} {tag}] max error / bound = {r:.3f} over {got.numel()} elements")
    WORST[entry] = max(WORST[entry], r)
    assert r <= 1.0, (entry, tag, r)
    return r


class Out:
    """n elements of the sentinel (or `init`) between two 16-byte-keeping guard bands of the sentinel."""

    def __init__(self, n, dev, dtype=torch.float32, init=None):
        self.n = n
        self.buf, self.v = R.guarded(n, dtype=dtype, device=dev, guard=R.AGUARD)
        if init is not None:
            self.v.copy_(init.reshape(-1))

    def intact(self):
        return R.guard_intact(self.buf, self.n, guard=R.AGUARD)

    def untouched(self):
        return bool((self.buf == R.SENTINEL).all())


def _twice(tag, run):
    """run() -> tuple of Out, on fresh buffers each time: bit-identical, guard bands intact."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for oa, ob in zip(a, b):
        assert torch.equal(oa.buf, ob.buf), f"{tag}: two runs differ"
        assert oa.intact(), f"{tag}: wrote outside its destination"
    return a


def _api():
    from semivl_amd import ops
    return ops, ops.L.load(), ops._p, ops._st


def _dev(tensors, dev):
    return [t.to(dev) if torch.is_tensor(t) else t for t in tensors]


def _ok(rc, L):
    assert rc == 0, L.last_error()


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def _ln_fwd_case(dev, rows, C):
    ops, lib, p, st = _api()
    x, dy, add, gamma, beta, eps = _dev(R.ln_inputs(rows, C), dev)
    tag = f"{rows}x{C}"

    def run():
        y, s = Out(rows * C, dev), Out(rows * 2, dev)
        _ok(lib.svl_layernorm_fwd(p(x), p(gamma), p(beta), eps, rows, C, p(y.v), p(s.v), st()), ops.L)
        return y, s
    y, s = _twice(tag, run)
    w = R.ln_fwd_ref(x, gamma, beta, eps)
    _ratio("svl_layernorm_fwd", f"y {tag}", y.v.view(rows, C), w["y"], w["dy_"])
    _ratio("svl_layernorm_fwd", f"stats {tag}", s.v.view(rows, 2), w["stats"], w["dstats"])


@pytest.mark.parametrize("C", R.LN_FWD_C)
def test_layernorm_fwd(dev, C):
    for rows in R.LN_FWD_ROWS:
        _ln_fwd_case(dev, rows, C)


def test_layernorm_fwd_second_grid_trip(dev):
    _ln_fwd_case(dev, *R.LN_FWD_BIG)


def _ln_planes_case(dev, rows, C):
    """Both plane-emitting forms: y and stats under the bounds; the planes are split_planes of the device's own y bit for bit,
    the padding rows of the last 32-row block zero, nothing behind it written; sexp is the exponent of max |y|, rnorm an upper
    bound of the row norm within 1e-4 (the condition of test_ops_gpu.py::test_layernorm_emits_planes), both untouched from
    `rows` on; y = NULL gives the same planes, stats, sexp and rnorm."""
    ops, lib, p, st = _api()
    x, dy, add, gamma, beta, eps = _dev(R.ln_inputs(rows, C), dev)
    w = R.ln_fwd_ref(x, gamma, beta, eps)
    prow, nblk = R.planes_rows_ref(rows), (rows + 31) // 32
    assert prow == ops.planes_rows(rows)
    for fmt, per, dt in (("b3", 48, torch.bfloat16), ("h2", 32, torch.float16)):
        tag = f"{fmt} {rows}x{C}"
        entry = "svl_layernorm_fwd_planes" + ("_f16x2" if fmt == "h2" else "")

        def run(with_y):
            def f():
                y, s, pl = Out(rows * C, dev), Out(rows * 2, dev), Out(C // 16 * prow * per, dev, dt)
                se, rn = Out(prow, dev, torch.int32), Out(prow, dev)
                yp = p(y.v) if with_y else None
                if fmt == "b3":
                    rc = lib.svl_layernorm_fwd_planes(p(x), p(gamma), p(beta), eps, rows, C, yp, p(s.v), p(pl.v), prow, st())
                else:
                    rc = lib.svl_layernorm_fwd_planes_f16x2(p(x), p(gamma), p(beta), eps, rows, C, yp, p(s.v), p(pl.v), prow,
                                                            p(se.v), p(rn.v), st())
                _ok(rc, ops.L)
                return y, s, pl, se, rn
            return f
        y, s, pl, se, rn = _twice(tag, run(True))
        y0, s0, pl0, se0, rn0 = _twice(tag + " y=NULL", run(False))
        assert y0.untouched() and all(torch.equal(a.buf, b.buf) for a, b in ((s0, s), (pl0, pl), (se0, se), (rn0, rn))), tag
        yv = y.v.view(rows, C)
        _ratio(entry, f"y {tag}", yv, w["y"], w["dy_"])
        _ratio(entry, f"stats {tag}", s.v.view(rows, 2), w["stats"], w["dstats"])
        ref, rse = Out(pl.n, dev, dt), Out(prow, dev, torch.int32)
        ops.split_planes(yv, out=ops.Planes(rows, C, buf=ref.v, fmt=fmt, sexp=rse.v if fmt == "h2" else None))
        pv, rv = R.planes_view(pl.v, C, prow, fmt), R.planes_view(ref.v, C, prow, fmt)
        assert torch.equal(pv[:, :nblk], rv[:, :nblk]), f"{tag}: planes differ from split_planes(y)"
        assert bool((pv[:, nblk:] == R.SENTINEL).all()), f"{tag}: row blocks beyond the last one written"
        if rows % 32:
            assert bool((pv[:, nblk - 1, :, :, rows % 32:, :] == 0).all()), f"{tag}: padding rows of the last block not zero"
        if fmt == "h2":
            assert torch.equal(se.v[:rows], R.sexp_ref(yv)) and torch.equal(se.v[:rows], rse.v[:rows]), f"{tag}: sexp"
            nrm = yv.double().norm(dim=1)
            assert bool((rn.v[:rows].double() >= nrm).all()) and bool((rn.v[:rows].double() <= nrm * (1 + 1e-4)).all()), f"{tag}: rnorm"
            assert bool((se.v[rows:] == int(R.SENTINEL)).all()) and bool((rn.v[rows:] == R.SENTINEL).all()), f"{tag}: padding scales written"
        else:
            assert se.untouched() and rn.untouched()


@pytest.mark.parametrize("C", R.LN_PLANES_C)
def test_layernorm_fwd_planes(dev, C):
    for rows in R.LN_PLANES_ROWS:
        _ln_planes_case(dev, rows, C)


def test_layernorm_fwd_planes_second_grid_trip(dev):
    _ln_planes_case(dev, *R.LN_PLANES_BIG)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_bwd_case(dev, rows, C, parts):
    """svl_layernorm_bwd on the device's own stats (fed to both sides), with and without dx_add; parts: also with the
    weight-gradient partials, whose dx must be the bits of the form without them; dgamma / dbeta = ops.colsum of the slabs."""
    ops, lib, p, st = _api()
    x, dy, add, gamma, beta, eps = _dev(R.ln_inputs(rows, C), dev)
    y, stats = torch.empty_like(x), torch.empty(rows, 2, device=dev)
    _ok(lib.svl_layernorm_fwd(p(x), p(gamma), p(beta), eps, rows, C, p(y), p(stats), st()), ops.L)
    nparts = lib.svl_layernorm_bwd_parts(rows)
    assert nparts == R.ln_parts_ref(rows)

    def run(a, with_parts):
        def f():
            dx = Out(rows * C, dev)
            dg, db = (Out(nparts * C, dev), Out(nparts * C, dev)) if with_parts else (None, None)
            _ok(lib.svl_layernorm_bwd(p(dy), p(x), p(stats), p(gamma), rows, C, p(a), p(dx.v), p(dg.v) if dg else None,
                                      p(db.v) if db else None, st()), ops.L)
            return (dx, dg, db) if with_parts else (dx,)
        return f
    for a, name in ((add, "dx_add"), (None, "no dx_add")):
        tag = f"{rows}x{C} {name}"
        w = R.ln_bwd_ref(dy, x, stats, gamma, a)
        dx = _twice(tag, run(a, False))[0]
        _ratio("svl_layernorm_bwd", f"dx {tag}", dx.v.view(rows, C), w["dx"], w["ddx"])
        if parts:
            dxp, dg, db = _twice(tag + " parts", run(a, True))
            assert torch.equal(dxp.buf, dx.buf), f"{tag}: dx of the form with partials differs"
            _ratio("svl_layernorm_bwd", f"dgamma {tag}", ops.colsum(dg.v.view(nparts, C)), w["dgamma"], w["ddgamma"])
            _ratio("svl_layernorm_bwd", f"dbeta {tag}", ops.colsum(db.v.view(nparts, C)), w["dbeta"], w["ddbeta"])


@pytest.mark.parametrize("C", R.LN_BWD_C)
def test_layernorm_bwd(dev, C):
    for rows in R.LN_BWD_ROWS:
        _ln_bwd_case(dev, rows, C, False)
    for rows in R.LN_BWD_ROWS_PARTS:
        _ln_bwd_case(dev, rows, C, True)


def test_layernorm_bwd_long_blocks(dev):
    """2048 blocks of 65 rows; dy lives in five rows (tests/test_rownorm_ref.py shows a dropped one leaves the bound by > 10 x)."""
    _ln_bwd_case(dev, *R.LN_BWD_BIG, True)


# ------------------------------------------------------------------------------------------------ row softmax
def _softmax_case(dev, rows, cols, ld, scale):
    ops, lib, p, st = _api()
    s, dp = _dev(R.sm_inputs(rows, cols, ld, scale), dev)
    tag = f"{rows}x{cols} ld {ld} scale {scale}"

    def fwd():
        o = Out(rows * ld, dev, init=s)
        ops.softmax_rows_fwd(o.v, rows, cols, ld, scale)
        return (o,)
    (o,) = _twice(tag, fwd)
    pv = o.v.view(rows, ld)
    w, bw = R.softmax_fwd_ref(s, cols, scale)
    _ratio("svl_softmax_rows_fwd", tag, pv, w, bw)                      # (bound 0 in [cols, ld): exact zeros)
    assert bool(((pv.double().sum(1) - 1.0).abs() <= bw.sum(1)).all()), f"{tag}: row sums"
    keep = o.buf.clone()

    def bwd():
        d = Out(rows * ld, dev, init=dp)
        ops.softmax_rows_bwd(d.v, pv, rows, cols, ld, scale)
        return (d,)
    (d,) = _twice(tag + " bwd", bwd)
    g, bg = R.softmax_bwd_ref(dp, pv, cols, scale)
    _ratio("svl_softmax_rows_bwd", tag, d.v.view(rows, ld), g, bg)
    assert torch.equal(o.buf, keep), f"{tag}: p was written"


@pytest.mark.parametrize("cols", R.SM_COLS)
def test_softmax_rows(dev, cols):
    for ld in R.sm_lds(cols):
        for rows in R.SM_ROWS:
            for scale in R.SM_SCALES:
                _softmax_case(dev, rows, cols, ld, scale)


def test_softmax_rows_second_grid_trip(dev):
    _softmax_case(dev, *R.SM_BIG, 0.125)


# ------------------------------------------------------------------------------------------------ L2 normalisation
def _l2_case(dev, rows, C, eps):
    ops, lib, p, st = _api()
    x, dy, kinds = _dev(R.l2_inputs(rows, C, eps), dev)
    tag = f"{rows}x{C} eps {eps} {kinds[:5]}"

    def fwd():
        y, inv = Out(rows * C, dev), Out(rows, dev)
        _ok(lib.svl_l2norm_fwd(p(x), rows, C, eps, p(y.v), p(inv.v), st()), ops.L)
        return y, inv
    y, inv = _twice(tag, fwd)
    w = R.l2norm_fwd_ref(x, eps)
    _ratio("svl_l2norm_fwd", f"y {tag}", y.v.view(rows, C), w["y"], w["dy_"])
    _ratio("svl_l2norm_fwd", f"inv {tag}", inv.v, w["inv"], w["dinv"])

    def bwd():
        dx = Out(rows * C, dev)
        _ok(lib.svl_l2norm_bwd(p(dy), p(y.v), p(inv.v), rows, C, p(dx.v), st()), ops.L)
        return (dx,)
    (dx,) = _twice(tag + " bwd", bwd)
    _ratio("svl_l2norm_bwd", tag, dx.v.view(rows, C), *R.l2norm_bwd_ref(dy, y.v.view(rows, C), inv.v))


@pytest.mark.parametrize("C", R.L2_C)
def test_l2norm(dev, C):
    for rows in R.L2_ROWS:
        for eps in R.L2_EPS:
            _l2_case(dev, rows, C, eps)


def test_l2norm_second_grid_trip(dev):
    for eps in R.L2_EPS:
        _l2_case(dev, *R.L2_BIG, eps)


# ------------------------------------------------------------------------------------------------ column sums
def _colsum_case(dev, name, rows, C, ld, off, floats):
    """x = the column slice at column `off` of a [rows, ld] matrix of -sentinel (off % 4 != 0: a pointer off 16-byte alignment).
    Integer-valued data: equality, accumulate 0 and 1; N(0, 1) and cancellation data (floats): the bound."""
    ops, lib, p, st = _api()
    assert lib.svl_colsum_ws_floats(rows, C) == min(1024, (rows + 255) // 256) * C
    buf, xv = R.strided(rows, C, ld, off, dev, fill=-R.SENTINEL)
    assert (xv.data_ptr() % 16 == 0) == (off % 4 == 0)

    def put(t):
        xv.copy_(t.to(dev))
        return buf.clone()

    def run(base):
        def f():
            o = Out(C, dev, init=base)
            ops.colsum(xv, out=o.v, accumulate=base is not None, C_=C, ld=ld)
            return (o,)
        return f
    tag = f"{name} {rows}x{C} ld {ld}"
    base_i = R.cs_ints(1, C, seed=1)[0].to(dev)
    keep = put(R.cs_ints(rows, C))
    want, _ = R.colsum_ref(xv)
    for base in (None, base_i):
        (o,) = _twice(tag, run(base))
        assert torch.equal(o.v.double(), want + (base.double() if base is not None else 0)), f"{tag}: integer sums (accumulate {base is not None})"
    assert torch.equal(buf, keep), f"{tag}: x or its surroundings were written"
    WORST["svl_colsum_f32 (integer data: equal)"] = 0.0
    if floats:
        base_f = torch.randn(C, generator=torch.Generator().manual_seed(C)).to(dev)
        for kind, t in zip(("n01", "cancel"), R.cs_floats(rows, C)):
            keep = put(t)
            for base in (None, base_f):
                (o,) = _twice(tag, run(base))
                _ratio("svl_colsum_f32", f"{kind} accumulate {int(base is not None)} {tag}", o.v, *R.colsum_ref(xv, base=base))
            assert torch.equal(buf, keep)


@pytest.mark.parametrize("layout", R.CS_LAYOUTS, ids=lambda c: c[0])
def test_colsum(dev, layout):
    name, C, ld, off = layout
    for rows in R.CS_ROWS:
        _colsum_case(dev, name, rows, C, ld, off, True)


def test_colsum_chunk_cap_and_long_column(dev):
    ops, lib, p, st = _api()
    name, rows, C, ld, off = R.CS_BIG
    _colsum_case(dev, name, rows, C, ld, off, False)
    # one long column: ops.colsum sums it as a [rows / 1024, 1024] matrix, then 1024 values
    x = R.cs_ints(R.CS_LONG, 1).to(dev)
    a, b = ops.colsum(x), ops.colsum(x)
    assert torch.equal(a, b) and torch.equal(a.double(), x.double().sum(0))
    o = Out(1, dev, init=torch.tensor([5.0]))
    ops.colsum(x, out=o.v, accumulate=True)
    assert o.intact() and float(o.v[0]) == float(x.double().sum()) + 5.0


# ------------------------------------------------------------------------------------------------ exact movers
def test_exact_movers(dev):
    ops, lib, p, st = _api()
    for outer, A, B, C in R.PERMUTE_CASES:
        n = outer * A * B
        x = torch.randn(n, C, generator=torch.Generator().manual_seed(n)).to(dev)

        def perm():
            o = Out(n * C, dev)
            _ok(lib.svl_permute_rows_f32(p(x), outer, A, B, C, p(o.v), st()), ops.L)
            return (o,)
        (o,) = _twice(f"permute_rows {outer, A, B, C}", perm)
        assert torch.equal(o.v.view(n, C), R.permute_rows_ref(x, outer, A, B, C))
    assert max(o_ * a * b for o_, a, b, _ in R.PERMUTE_CASES) > 4 * 8192
    for rows, rpi, C in R.CHANMASK_CASES:
        g = torch.Generator().manual_seed(rows)
        x = torch.randn(rows, C, generator=g).to(dev)
        mask = (torch.rand((rows + rpi - 1) // rpi, C, generator=g) < 0.5).float().to(dev)

        def cm():
            o = Out(rows * C, dev)
            ops.chanmask(x, mask, 2.0, rpi, out=o.v)
            return (o,)
        (o,) = _twice(f"chanmask {rows, rpi, C}", cm)
        assert torch.equal(o.v.view(rows, C), R.chanmask_ref(x, mask, 2.0, rpi))
    for rows in R.BOUND2_ROWS:
        g = torch.Generator().manual_seed(rows)
        rn, bias = torch.rand(rows, generator=g), torch.randn(rows + 2, generator=g)
        rn[-1], bias[-1] = 3.0, -5.0                    # the maximum in the last element
        rn, bias = rn.to(dev), bias.to(dev)
        for b in (bias, None):
            def b2():
                o = Out(2, dev)
                _ok(lib.svl_bound2_f32(p(rn), rows, p(b), b.numel() if b is not None else 0, p(o.v), st()), ops.L)
                return (o,)
            (o,) = _twice(f"bound2 {rows}", b2)
            assert torch.equal(o.v, R.bound2_ref(rn, b)) and float(o.v[0]) == 3.0 and float(o.v[1]) == (5.0 if b is not None else 0.0)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(L, rc, code, pattern, *outs):
    assert rc == code, (rc, code, pattern)
    assert re.search(pattern, L.last_error()), (pattern, L.last_error())
    torch.cuda.synchronize()
    for o in outs:
        assert o.untouched(), f"a refused call wrote its output ({pattern})"


def test_refusals(dev):
    """By return code and message only; nothing is written."""
    ops, lib, p, st = _api()
    L = ops.L
    rows = 10
    S = lambda n, dt=torch.float32: Out(n, dev, dt)
    x, y, dy, dx, g, b, stats = S(rows * 1028), S(rows * 1028), S(rows * 1028), S(rows * 1028), S(1028), S(1028), S(rows * 2)
    pl, se, rn, dg, db = S(1028 // 16 * 512 * 48, torch.float16), S(512, torch.int32), S(512), S(1028), S(1028)
    outs = (y, dx, stats, pl, se, rn, dg, db)
    xv, yv, dyv, dxv, gv, bv, sv = p(x.v), p(y.v), p(dy.v), p(dx.v), p(g.v), p(b.v), p(stats.v)
    # C % 4 != 0
    _refused(L, lib.svl_layernorm_fwd(xv, gv, bv, 1e-5, rows, 6, yv, sv, st()), -1, "svl_layernorm_fwd", *outs)
    # the plane-emitting forms: C % 16 != 0, planes_rows not a multiple of 256, planes_rows below rows
    for C, nrows, prow in ((8, rows, 256), (16, rows, 300), (16, 300, 256)):
        _refused(L, lib.svl_layernorm_fwd_planes(xv, gv, bv, 1e-5, nrows, C, yv, sv, p(pl.v), prow, st()), -1, "svl_layernorm_fwd_planes", *outs)
        _refused(L, lib.svl_layernorm_fwd_planes_f16x2(xv, gv, bv, 1e-5, nrows, C, yv, sv, p(pl.v), prow, p(se.v), p(rn.v), st()), -1,
                 "svl_layernorm_fwd_planes_f16x2", *outs)
    # the fp16 x 2 form without sexp
    _refused(L, lib.svl_layernorm_fwd_planes_f16x2(xv, gv, bv, 1e-5, rows, 16, yv, sv, p(pl.v), 256, None, p(rn.v), st()), -1, "sexp required", *outs)
    # backward: C above 1024; one of the two partial pointers alone
    _refused(L, lib.svl_layernorm_bwd(dyv, xv, sv, gv, rows, 1028, None, dxv, None, None, st()), -1, r"svl_layernorm_bwd.*C=1028", *outs)
    _refused(L, lib.svl_layernorm_bwd(dyv, xv, sv, gv, rows, 16, None, dxv, p(dg.v), None, st()), -1, "go together", *outs)
    _refused(L, lib.svl_layernorm_bwd(dyv, xv, sv, gv, rows, 16, None, dxv, None, p(db.v), st()), -1, "go together", *outs)
    # the one-pass forms serve C = 768 only
    for C in (16, 752, 784, 1024):
        _refused(L, lib.svl_layernorm_fwd_pack_f16x2(xv, gv, bv, 1e-5, rows, C, yv, sv, p(pl.v), 256, 0, p(se.v), p(rn.v), 0, None, st()), -3,
                 "svl_layernorm_fwd_pack_f16x2.*768", *outs)
        _refused(L, lib.svl_layernorm_bwd_pack_f16x2(dyv, xv, sv, gv, rows, C, None, dxv, p(pl.v), 256, 0, p(se.v), p(rn.v), None, st()), -3,
                 "svl_layernorm_bwd_pack_f16x2.*768", *outs)
    # a row stride below the row
    _refused(L, lib.svl_softmax_rows_fwd(yv, rows, 8, 7, 1.0, st()), -1, "svl_softmax_rows_fwd", *outs)
    _refused(L, lib.svl_softmax_rows_bwd(dxv, xv, rows, 8, 7, 1.0, st()), -1, "svl_softmax_rows_bwd", *outs)
    _refused(L, lib.svl_colsum_f32(xv, rows, 8, 7, p(dg.v), 0, p(db.v), st()), -1, "svl_colsum_f32", *outs)
    # permute_rows: a pointer off 16-byte alignment, source and destination in turn
    _refused(L, lib.svl_permute_rows_f32(x.v.data_ptr() + 4, 1, 2, 3, 4, dxv, st()), -1, "svl_permute_rows_f32", *outs)
    _refused(L, lib.svl_permute_rows_f32(xv, 1, 2, 3, 4, dx.v.data_ptr() + 4, st()), -1, "svl_permute_rows_f32", *outs)


def test_layernorm_alignment_refusals(dev):
    """The LayerNorm kernels read and write x / y / gamma / beta / dy / dx / dx_add as 16-byte quads: a pointer 4 bytes off,
    inside a larger valid allocation, is refused by each of the six entry points before anything is launched -- each operand in
    turn, by return code and message; nothing is written."""
    ops, lib, p, st = _api()
    L = ops.L
    rows, C, prow = 32, 768, 256
    S = lambda n, dt=torch.float32: Out(n, dev, dt)
    x, y, dy, dx, add, g, b = [S(rows * C + 4) for _ in range(5)] + [S(C + 4), S(C + 4)]
    stats, pl, se, rn = S(rows * 2), S(C // 16 * prow * 48, torch.float16), S(prow, torch.int32), S(prow)
    outs = (y, dx, stats, pl, se, rn)
    a = lambda o, off: o.v.data_ptr() + 4 * off
    msg = "16-byte aligned"
    for k in range(4):          # x, y, gamma, beta
        o = [1 if i == k else 0 for i in range(4)]
        X, Y, G, B = a(x, o[0]), a(y, o[1]), a(g, o[2]), a(b, o[3])
        _refused(L, lib.svl_layernorm_fwd(X, G, B, 1e-5, rows, C, Y, p(stats.v), st()), -1, msg, *outs)
        _refused(L, lib.svl_layernorm_fwd_planes(X, G, B, 1e-5, rows, C, Y, p(stats.v), p(pl.v), prow, st()), -1, msg, *outs)
        _refused(L, lib.svl_layernorm_fwd_planes_f16x2(X, G, B, 1e-5, rows, C, Y, p(stats.v), p(pl.v), prow, p(se.v), p(rn.v), st()), -1, msg, *outs)
        _refused(L, lib.svl_layernorm_fwd_pack_f16x2(X, G, B, 1e-5, rows, C, Y, p(stats.v), p(pl.v), prow, 0, p(se.v), p(rn.v), 0, None, st()), -1,
                 msg, *outs)
    for k in range(5):          # dy, x, gamma, dx_add, dx
        o = [1 if i == k else 0 for i in range(5)]
        D, X, G, A, DX = a(dy, o[0]), a(x, o[1]), a(g, o[2]), a(add, o[3]), a(dx, o[4])
        _refused(L, lib.svl_layernorm_bwd(D, X, p(stats.v), G, rows, C, A, DX, None, None, st()), -1, msg, *outs)
        _refused(L, lib.svl_layernorm_bwd_pack_f16x2(D, X, p(stats.v), G, rows, C, A, DX, p(pl.v), prow, 0, p(se.v), p(rn.v), None, st()), -1,
                 msg, *outs)
