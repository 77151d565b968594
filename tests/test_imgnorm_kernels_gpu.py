"""GPU: the channels-last image normalisations -- the GroupNorm family of csrc/norm.hip (svl_groupnorm_fwd / _apply /
_scale_shift / _bwd / _bwd_apply) and the BatchNorm chain of csrc/batchnorm.hip (svl_bn_stats / _finalize / _eval_invstd /
_apply / _bwd_reduce / _bwd_apply) -- each through semivl_amd.ops against the float64 restatements of tests/imgnorm_ref.py
under the bounds derived there: no tolerance is chosen here.

Every case passes every operand that has a stride as a column slice at a non-zero 16-byte aligned offset of a wider
sentinel matrix, with a different row stride for every operand; the gap columns and guard bands must come back intact;
everything runs twice for a bit-for-bit comparison; where a ReLU is fused, the form that reads y and the form that re-derives
the mask from x must agree bit for bit; -s prints max error / bound, which has to be <= 1.  The inputs are built so that no
ReLU mask is undecided (tests/test_imgnorm_ref.py asserts it), so no element is left out of a comparison.

The shapes reach what the usual N(0, 1), C in {32 .. 256} cases do not: the scalar tails of the unrolled loops, HW below the
pixel rows of a block, both sides of the 256 / 1024-thread switch, the second trip of a capped grid, channel counts that
leave lanes idle, the chunk cap of the two-stage reductions, and every argument refusal."""
import collections

import numpy as np
import pytest
import torch

import imgnorm_ref as R

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


class Src:
    """t2d [rows, C] as a column slice at column `off` of a [rows, ld] matrix of -SENTINEL; intact(): nothing moved."""

    def __init__(self, t2d, ld, off, dev):
        self.rows, self.C, self.ld, self.off = t2d.shape[0], t2d.shape[1], ld, off
        self.buf, self.v = R.strided(self.rows, self.C, ld, off, dev, fill=-R.SENTINEL)
        self.v.copy_(t2d)
        self.keep = self.buf.clone()

    def intact(self):
        return torch.equal(self.buf, self.keep)


def _twice(tag, make, run, intact):
    """run(view) on two fresh (buffer, view) pairs: bit-identical buffers and results, guard bands intact.  Returns
    (view, result of run)."""
    out = []
    for _ in range(2):
        buf, v = make()
        out.append((buf, v, run(v)))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]), f"{tag}: two runs differ"
    ra, rb = out[0][2], out[1][2]
    if ra is not None:
        for a, b in zip(ra if isinstance(ra, tuple) else (ra,), rb if isinstance(rb, tuple) else (rb,)):
            assert torch.equal(a, b), f"{tag}: two runs differ"
    assert intact(out[0][0]), f"{tag}: wrote outside its destination"
    return out[0][1], ra


def _void(f):
    return lambda v: (f(v), None)[1]


def _dst(rows, C, ld, off, dev):
    return (lambda: R.strided(rows, C, ld, off, dev)), (lambda buf: R.gaps_intact(buf, rows, C, ld, off))


def _flat(n, dev, init=None, dtype=torch.float32):
    def make():
        buf, v = R.guarded(n, dtype=dtype, device=dev, guard=R.AGUARD)
        if init is not None:
            v.copy_(init.reshape(-1))
        return buf, v
    return make, (lambda buf: R.guard_intact(buf, n, guard=R.AGUARD))


# ------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: c[0])
def test_groupnorm_family(dev, case):
    """svl_groupnorm_fwd, _apply (the same bits), _scale_shift, _bwd with the mask read from y and re-derived from x (the same
    bits), _bwd_apply on the channel sums _bwd left (the same bits), dgamma / dbeta of the wrappers, all under the derived bounds.

    The constant image (x = 3.0): the statistics are bit-defined (mean 3, variance exactly 0, rstd = fl(1 / sqrt(eps))) and are
    compared for equality; the restatement's y is beta (relu(beta)) exactly.  The kernel's y is NOT beta to the bit, and cannot be
    under the header's affine form: sh = fma(-mean, sc, beta) is rounded at the magnitude of mean * sc (about 950), so
    y = fma(x, sc, sh) = beta + e with |e| <= U |mean sc|: a plain fp32 evaluation on the CPU gives max |y - beta| = 5.8e-5 with
    nearly every element off beta.  y is therefore held to the derived bound there like everywhere else (measured ratio 0.10)."""
    from semivl_amd import ops
    name, imgs, HW, C, G, relu, variant = case
    x, dy, gamma, beta = [t.to(dev) for t in R.gn_inputs(case)]
    rows = imgs * HW
    ldx, ldy, lddy, lddx, ldy2, lddx2 = C + 4, C + 8, C + 12, C + 16, C + 20, C + 24
    xs, dys = Src(x.view(rows, C), ldx, 4, dev), Src(dy.view(rows, C), lddy, 8, dev)
    fwd = R.gn_fwd_ref(x, gamma, beta, G, relu)
    bwd = R.gn_bwd_ref(x, dy, fwd, gamma)
    shape = (imgs, HW, C)

    # forward: statistics and y
    mk, ok = _dst(rows, C, ldy, 4, dev)
    y, stats = _twice(name, mk, lambda v: ops.groupnorm_fwd(xs.v, ldx, gamma, beta, R.EPS, imgs, HW, C, G, relu, v, ldy), ok)
    _ratio("svl_groupnorm_fwd", f"stats {name}", stats, *R.gn_stats_pair(fwd["st"]))
    _ratio("svl_groupnorm_fwd", f"y {name}", y.reshape(shape), fwd["y"], fwd["bound"])
    if variant == "const":      # variance exactly 0: the statistics are bit-defined
        assert bool((stats[..., 0] == R.GN_CONST).all()) and bool((stats[..., 1] == float(np.float32(1 / np.sqrt(R.EPS)))).all())
    # the apply pass alone on the same statistics: the same bits
    mk, ok = _dst(rows, C, ldy2, 16, dev)
    y2, _ = _twice(name + " apply", mk, _void(lambda v: ops.groupnorm_apply(xs.v, ldx, gamma, beta, imgs, HW, C, G, relu, stats, v, ldy2)), ok)
    assert torch.equal(y2, y), f"{name}: svl_groupnorm_apply differs from svl_groupnorm_fwd"
    # the (scale, shift) table
    t1, t2 = (ops.groupnorm_scale_shift(stats, gamma, beta, imgs, C, G) for _ in range(2))
    assert torch.equal(t1, t2)
    _ratio("svl_groupnorm_scale_shift", name, t1, *R.gn_table_ref(fwd["st"], gamma, beta))

    # backward, mask read from y
    def run_bwd(beta_):
        def run(v):
            cs = torch.full((imgs, 2, C), R.SENTINEL, device=dev)
            dg, db = ops.groupnorm_bwd(dys.v, lddy, xs.v, ldx, None if beta_ is not None else y, ldy, stats, gamma, imgs, HW, C, G,
                                       relu, v, lddx, beta=beta_, cs=cs)
            return cs, dg, db
        return run
    mk, ok = _dst(rows, C, lddx, 12, dev)
    dx, (cs, dg, db) = _twice(name + " bwd", mk, run_bwd(None), ok)
    _ratio("svl_groupnorm_bwd", f"chan_sums {name}", cs, bwd["cs"], bwd["dcs"])
    _ratio("svl_groupnorm_bwd", f"dx {name}", dx.reshape(shape), bwd["dx"], bwd["ddx"])
    _ratio("svl_groupnorm_bwd", f"dgamma {name}", dg, bwd["dgamma"], bwd["ddgamma"])
    _ratio("svl_groupnorm_bwd", f"dbeta {name}", db, bwd["dbeta"], bwd["ddbeta"])
    # ... and re-derived from x: the forward's own decision, bit for bit
    dxr, (csr, dgr, dbr) = _twice(name + " bwd remask", mk, run_bwd(beta), ok)
    assert torch.equal(dxr, dx) and torch.equal(csr, cs) and torch.equal(dgr, dg) and torch.equal(dbr, db), f"{name}: remask form"
    # the apply pass alone on the channel sums svl_groupnorm_bwd left
    mk, ok = _dst(rows, C, lddx2, 20, dev)
    dxa, (dga, dba) = _twice(name + " bwd_apply", mk, lambda v: ops.groupnorm_bwd_from_sums(
        dys.v, lddy, xs.v, ldx, stats, gamma, beta, imgs, HW, C, G, relu, cs, v, lddx2), ok)
    assert torch.equal(dxa, dx) and torch.equal(dga, dg) and torch.equal(dba, db), f"{name}: svl_groupnorm_bwd_apply"
    WORST["svl_groupnorm_apply (bit-identical to _fwd)"] = 0.0
    WORST["svl_groupnorm_bwd_apply (bit-identical to _bwd)"] = 0.0
    assert xs.intact() and dys.intact(), f"{name}: an input was written"


def _refused(fn, *bufs):
    """fn raises the bad-argument error and leaves every buffer full of its sentinel."""
    with pytest.raises(RuntimeError, match=r"status -1"):
        fn()
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == R.SENTINEL).all()), "a refused call wrote its output"


def _gn_calls(ops, dev, C, G, ld, imgs, HW, sx=0, sy=0, sd=0, sg=0, sgam=0, sbet=0):
    """{name: (call, outputs)} of the five strided GroupNorm entry points (svl_groupnorm_bwd in both forms) on sentinel
    buffers of [imgs * HW, ld]; s*: that operand starts so many floats off its 16-byte aligned buffer."""
    n = imgs * HW
    x, y, dy, dx = (torch.full((n * max(ld, C) + 4,), R.SENTINEL, device=dev) for _ in range(4))
    gam, bet = torch.full((C + 4,), R.SENTINEL, device=dev), torch.full((C + 4,), R.SENTINEL, device=dev)
    stats = torch.zeros(imgs, max(G, 1), 2, device=dev)
    cs = torch.full((imgs, 2, C), R.SENTINEL, device=dev)
    x_, y_, dy_, dx_, g, b = x[sx:], y[sy:], dy[sd:], dx[sg:], gam[sgam:], bet[sbet:]
    return {
        "fwd": (lambda: ops.groupnorm_fwd(x_, ld, g, b, R.EPS, imgs, HW, C, G, True, y_, ld), (y,)),
        "apply": (lambda: ops.groupnorm_apply(x_, ld, g, b, imgs, HW, C, G, True, stats, y_, ld), (y,)),
        "bwd_y": (lambda: ops.groupnorm_bwd(dy_, ld, x_, ld, y_, ld, stats, g, imgs, HW, C, G, True, dx_, ld, cs=cs), (dx, cs)),
        "bwd_remask": (lambda: ops.groupnorm_bwd(dy_, ld, x_, ld, None, 0, stats, g, imgs, HW, C, G, True, dx_, ld, beta=b, cs=cs),
                       (dx, cs)),
        "bwd_apply": (lambda: ops.groupnorm_bwd_from_sums(dy_, ld, x_, ld, stats, g, b, imgs, HW, C, G, True, cs, dx_, ld), (dx,)),
        "scale_shift": (lambda: ops.groupnorm_scale_shift(stats, g, b, imgs, C, G), ()),
    }


STRIDED = ("fwd", "apply", "bwd_y", "bwd_remask", "bwd_apply")


def test_groupnorm_refusals(dev):
    """Bad shapes, strides, alignment and image counts come back as SVL_ERR_INVALID_ARG with nothing written."""
    from semivl_amd import ops
    imgs, HW = 2, 6

    def refuse(calls, names):
        for k in names:
            _refused(calls[k][0], *calls[k][1])

    for C, G in ((12, 1),              # 256 % CQ != 0
                 (2048, 64),           # CQ > 256
                 (256, 128),           # G > 64
                 (32, 16),             # (C / G) % 4 != 0
                 (32, 3)):             # C % G != 0
        refuse(_gn_calls(ops, dev, C, G, C, imgs, HW), STRIDED + ("scale_shift",))
    refuse(_gn_calls(ops, dev, 16, 4, 18, imgs, HW), STRIDED)          # ld % 4 != 0
    refuse(_gn_calls(ops, dev, 16, 4, 12, imgs, HW), STRIDED)          # ld < C
    # svl_groupnorm_bwd / _bwd_apply: each stride below C in turn
    C, G = 16, 4
    x, y, dyb, dx = (torch.full((imgs * HW * 20 + 4,), R.SENTINEL, device=dev) for _ in range(4))
    gam, bet = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    stats, cs = torch.zeros(imgs, G, 2, device=dev), torch.full((imgs, 2, C), R.SENTINEL, device=dev)
    for bad in (12, 8):
        for k in range(4):
            ld = [bad if i == k else 20 for i in range(4)]      # lddy, ldx, ldy, lddx
            _refused(lambda: ops.groupnorm_bwd(dyb, ld[0], x, ld[1], y, ld[2], stats, gam, imgs, HW, C, G, True, dx, ld[3], cs=cs), dx, cs)
            if k != 2:
                _refused(lambda: ops.groupnorm_bwd(dyb, ld[0], x, ld[1], None, 0, stats, gam, imgs, HW, C, G, True, dx, ld[3], beta=bet,
                                                   cs=cs), dx, cs)
                _refused(lambda: ops.groupnorm_bwd_from_sums(dyb, ld[0], x, ld[1], stats, gam, bet, imgs, HW, C, G, True, cs, dx, ld[3]), dx)
    # a pointer one float off 16-byte alignment: every operand that is read or written in channel quads, in turn
    refuse(_gn_calls(ops, dev, 16, 4, 16, imgs, HW, sx=1), STRIDED)
    refuse(_gn_calls(ops, dev, 16, 4, 16, imgs, HW, sy=1), ("fwd", "apply", "bwd_y"))
    refuse(_gn_calls(ops, dev, 16, 4, 16, imgs, HW, sd=1), ("bwd_y", "bwd_remask", "bwd_apply"))
    refuse(_gn_calls(ops, dev, 16, 4, 16, imgs, HW, sg=1), ("bwd_y", "bwd_remask", "bwd_apply"))
    refuse(_gn_calls(ops, dev, 16, 4, 16, imgs, HW, sgam=1), STRIDED + ("scale_shift",))
    refuse(_gn_calls(ops, dev, 16, 4, 16, imgs, HW, sbet=1), ("fwd", "apply", "bwd_remask", "bwd_apply", "scale_shift"))
    # more images than gridDim.y holds (HW = 1, C = 4: the smallest launch that would have been invalid)
    refuse(_gn_calls(ops, dev, 4, 1, 4, R.GN_MAX_IMGS + 1, 1), STRIDED)
    # ... and the largest count, which is taken
    n = R.GN_MAX_IMGS
    xx = torch.randn(n, 4, generator=torch.Generator().manual_seed(5)).to(dev)
    yy = torch.empty(n, 4, device=dev)
    one, zero = torch.ones(4, device=dev), torch.zeros(4, device=dev)
    st = ops.groupnorm_fwd(xx, 4, one, zero, R.EPS, n, 1, 4, 1, False, yy, 4)
    f = R.gn_fwd_ref(xx.view(n, 1, 4), one, zero, 1, False)
    _ratio("svl_groupnorm_fwd", "y imgs=65535", yy.view(n, 1, 4), f["y"], f["bound"])
    _ratio("svl_groupnorm_fwd", "stats imgs=65535", st, *R.gn_stats_pair(f["st"]))


# ------------------------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("case", R.BN_CASES, ids=lambda c: c[0])
def test_batchnorm_chain(dev, case):
    from semivl_amd import ops
    name, rows, C, relu, res, variant, momentum, running = case
    x, dy, gamma, beta, resid, rm, rv = [t.to(dev) if t is not None else None for t in R.bn_inputs(case)]
    ldx, ldr, ldy, lddy, lddx, lddr, ldye = C + 4, C + 8, C + 12, C + 16, C + 20, C + 24, C + 28
    xs, dys = Src(x, ldx, 4, dev), Src(dy, lddy, 12, dev)
    rs = Src(resid, ldr, 8, dev) if res else None
    f = R.bn_fwd_from_x(x, gamma, beta, resid, relu, momentum, rm if running else None, rv if running else None)
    mean_w, invstd_w = f["fin"]["mean"], f["fin"]["invstd"]
    b = R.bn_bwd_ref(x, dy, f["mask"], *mean_w, *invstd_w, gamma, rows)

    # statistics
    s1, s2 = ops.bn_stats(xs.v, C), ops.bn_stats(xs.v, C)
    assert torch.equal(s1, s2)
    _ratio("svl_bn_stats", name, s1, f["sums"], f["dsums"])
    # finalize: mean, invstd and the running statistics (or none)
    def fin(v):
        if not running:
            return ops.bn_finalize(s1, rows, R.EPS, momentum, None, None)
        return ops.bn_finalize(s1, rows, R.EPS, momentum, v[:C], v[C:])
    mk, ok = _flat(2 * C, dev, init=torch.cat((rm, rv)))
    run_stats, (mean, invstd) = _twice(name + " finalize", mk, fin, ok)
    _ratio("svl_bn_finalize", f"mean {name}", mean, *mean_w)
    _ratio("svl_bn_finalize", f"invstd {name}", invstd, *invstd_w)
    if running:
        _ratio("svl_bn_finalize", f"running_mean {name}", run_stats[:C], *f["fin"]["running_mean"])
        _ratio("svl_bn_finalize", f"running_var {name}", run_stats[C:], *f["fin"]["running_var"])
    else:
        assert torch.equal(run_stats, torch.cat((rm, rv)))
    if rows > 1:                # the constant channel: bit-defined statistics
        assert float(mean[3]) == R.BN_CONST and float(invstd[3]) == float(np.float32(1 / np.sqrt(R.EPS)))
    # apply (+ residual, + ReLU)
    mk, ok = _dst(rows, C, ldy, 4, dev)
    y, _ = _twice(name + " apply", mk, _void(lambda v: ops.bn_apply(xs.v, C, mean, invstd, gamma, beta, relu=relu,
                                                                 resid=rs.v if res else None, out=v)), ok)
    _ratio("svl_bn_apply", name, y, f["y"], f["bound"])
    if rows > 1 and not res:    # x - mean is exactly 0 there: y is beta (relu(beta)) to the bit
        assert bool((y[:, 3] == (beta[3].clamp_min(0) if relu else beta[3])).all())

    # backward sums and dx (+ dres), mask read from y
    yk = y if relu else None
    bs, bs2 = ops.bn_bwd_reduce(dys.v, xs.v, yk, C, mean, invstd), ops.bn_bwd_reduce(dys.v, xs.v, yk, C, mean, invstd)
    assert torch.equal(bs, bs2)
    _ratio("svl_bn_bwd_reduce", name, bs, b["sums"], b["dsums"])

    def run_dx(remask):
        def run(v):
            dx_v = v[:, :C]
            dres_v = R.strided(rows, C, lddr, 20, dev)
            out = ops.bn_bwd_apply(dys.v, xs.v, None if remask else yk, C, mean, invstd, gamma, bs, rows,
                                   remask_beta=beta if remask else None, dx_out=dx_v, dres_out=dres_v[1] if res else None)
            assert out[0].data_ptr() == dx_v.data_ptr() if res else out.data_ptr() == dx_v.data_ptr()
            return (dres_v[0],) if res else None
        return run
    mk, ok = _dst(rows, C, lddx, 16, dev)
    dx, extra = _twice(name + " bwd_apply", mk, run_dx(False), ok)
    _ratio("svl_bn_bwd_apply", f"dx {name}", dx, b["dx"], b["ddx"])
    if res:
        assert R.gaps_intact(extra[0], rows, C, lddr, 20)
        dres = extra[0][R.AGUARD:R.AGUARD + rows * lddr].view(rows, lddr)[:, 20:20 + C]
        _ratio("svl_bn_bwd_apply", f"dres {name}", dres, b["dres"], torch.zeros_like(b["dres"]))
    if relu and not res:        # the mask re-derived from x: bit for bit
        bsr = ops.bn_bwd_reduce(dys.v, xs.v, None, C, mean, invstd, remask=(gamma, beta))
        assert torch.equal(bsr, bs), f"{name}: remask sums"
        dxr, _ = _twice(name + " bwd_apply remask", mk, run_dx(True), ok)
        assert torch.equal(dxr, dx), f"{name}: remask dx"

    # eval mode: the running statistics the case started from
    inv_e = ops.bn_eval_invstd(rv, R.EPS)
    inv_w, dinv = R.bn_eval_invstd_ref(rv)
    _ratio("svl_bn_eval_invstd", name, inv_e, inv_w, dinv)
    pe, dpe, _ = R.bn_pre_ref(x, rm.double(), torch.zeros_like(inv_w), inv_w, dinv, gamma, beta)
    mk, ok = _dst(rows, C, ldye, 24, dev)
    ye, _ = _twice(name + " eval", mk, _void(lambda v: ops.bn_apply(xs.v, C, rm, inv_e, gamma, beta, out=v)), ok)
    _ratio("svl_bn_apply", f"eval {name}", ye, pe, dpe)
    assert xs.intact() and dys.intact() and (rs is None or rs.intact()), f"{name}: an input was written"


def test_batchnorm_shards(dev):
    """SyncBN: count != rows.  The sums of two shards finalised with count = all rows give the statistics of the whole batch;
    each shard's dx from the summed backward sums and that count is its rows of the whole batch's dx."""
    from semivl_amd import ops
    case = R.bn_case(R.BN_SHARD[0])
    k, (name, rows, C) = R.BN_SHARD[1], case[:3]
    x, dy, gamma, beta, resid, rm, rv = [t.to(dev) if t is not None else None for t in R.bn_inputs(case)]
    xs, dys = Src(x, C + 4, 4, dev), Src(dy, C + 16, 12, dev)
    f = R.bn_fwd_from_x(x, gamma, beta, None, True, 0.1, rm, rv)
    b = R.bn_bwd_ref(x, dy, f["mask"], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, rows)
    parts = (slice(0, k), slice(k, rows))
    s = ops.bn_stats(xs.v[parts[0]], C) + ops.bn_stats(xs.v[parts[1]], C)
    _ratio("svl_bn_stats", "two shards", s, f["sums"], f["dsums"])
    rmk, rvk = rm.clone(), rv.clone()
    mean, invstd = ops.bn_finalize(s, rows, R.EPS, 0.1, rmk, rvk)
    for tag, got in (("mean", mean), ("invstd", invstd), ("running_mean", rmk), ("running_var", rvk)):
        _ratio("svl_bn_finalize", f"{tag} two shards", got, *f["fin"][tag])
    y = torch.cat([ops.bn_apply(xs.v[p], C, mean, invstd, gamma, beta, relu=True) for p in parts])
    _ratio("svl_bn_apply", "two shards", y, f["y"], f["bound"])
    bs = sum(ops.bn_bwd_reduce(dys.v[p], xs.v[p], y[p], C, mean, invstd) for p in parts)
    _ratio("svl_bn_bwd_reduce", "two shards", bs, b["sums"], b["dsums"])
    for p in parts:
        dx = ops.bn_bwd_apply(dys.v[p], xs.v[p], y[p], C, mean, invstd, gamma, bs, rows)
        _ratio("svl_bn_bwd_apply", f"dx shard of {p.stop - p.start}", dx, b["dx"][p], b["ddx"][p])
        dxr = ops.bn_bwd_apply(dys.v[p], xs.v[p], None, C, mean, invstd, gamma, bs, rows, remask_beta=beta)
        assert torch.equal(dxr, dx)


def test_batchnorm_refusals(dev):
    from semivl_amd import ops
    rows, C = 10, 8
    S = lambda *shape: torch.full(shape, R.SENTINEL, device=dev)
    x, dy, y, dx, dres = (S(rows * C + 4) for _ in range(5))
    v = lambda t, off=0, c=C: t[off:off + rows * c].view(rows, c)
    mean, invstd, gamma, beta = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    sums = torch.zeros(2, C, dtype=torch.float64, device=dev)
    # C % 4 != 0
    m6 = torch.ones(6, device=dev)
    _refused(lambda: ops.bn_stats(v(x, 0, 6), 6))
    _refused(lambda: ops.bn_apply(v(x, 0, 6), 6, m6, m6, m6, m6, out=v(y, 0, 6)), y)
    _refused(lambda: ops.bn_bwd_reduce(v(dy, 0, 6), v(x, 0, 6), None, 6, m6, m6))
    _refused(lambda: ops.bn_bwd_apply(v(dy, 0, 6), v(x, 0, 6), None, 6, m6, m6, m6, sums, rows, dx_out=v(dx, 0, 6)), dx)
    # a pointer one float off 16-byte alignment, each operand in turn
    _refused(lambda: ops.bn_stats(v(x, 1), C))
    for ox, oy, orr in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        _refused(lambda: ops.bn_apply(v(x, ox), C, mean, invstd, gamma, beta, resid=v(dy, orr), out=v(y, oy)), y)
    for od, ox, oy in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        _refused(lambda: ops.bn_bwd_reduce(v(dy, od), v(x, ox), v(y, oy), C, mean, invstd))
    for od, ox, oy, odx, odr in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1)):
        _refused(lambda: ops.bn_bwd_apply(v(dy, od), v(x, ox), v(y, oy), C, mean, invstd, gamma, sums, rows,
                                          dx_out=v(dx, odx), dres_out=v(dres, odr)), dx, dres)
    # y together with remask_beta (the wrappers never pass both: the entry points themselves)
    lib, p, st = ops.L.load(), ops._p, ops._st()
    ws = torch.empty(int(lib.svl_bn_ws_doubles(rows, C)), dtype=torch.float64, device=dev)
    bsum = torch.full((2, C), R.SENTINEL, dtype=torch.float64, device=dev)
    rc = lib.svl_bn_bwd_reduce(p(dy), C, p(x), C, p(y), C, p(mean), p(invstd), p(gamma), p(beta), rows, C, p(bsum), p(ws), st)
    assert rc == -1
    rc = lib.svl_bn_bwd_apply(p(dy), C, p(x), C, p(y), C, p(mean), p(invstd), p(gamma), p(beta), p(sums), float(rows), rows, C,
                              p(dx), C, None, 0, st)
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((bsum == R.SENTINEL).all()) and bool((dx == R.SENTINEL).all())
    # count <= 0
    for count in (0, -3):
        _refused(lambda: ops.bn_finalize(sums, count, R.EPS, 0.1, mean, invstd))
        _refused(lambda: ops.bn_bwd_apply(v(dy), v(x), None, C, mean, invstd, gamma, sums, count, dx_out=v(dx)), dx)
    assert bool((mean == 0).all()) and bool((invstd == 1).all())
