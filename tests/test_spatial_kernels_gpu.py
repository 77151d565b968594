"""GPU: the memory-bound spatial kernels of the VLG head and the conv encoder (csrc/resample.hip, csrc/conv_thin.hip, the max
pool of csrc/batchnorm.hip), each through semivl_amd.ops against the float64 restatements of tests/spatial_ref.py (ATen only as
the checker) under the bounds derived there -- no tolerance is chosen here.

Every case is non-square in each pair of axes that could be exchanged, passes strided operands (a column slice at a
non-zero 16-byte aligned offset of a wider row) wherever the entry point takes a stride, writes into sentinel guard bands
(and the gap columns of a strided destination) that must come back intact, runs twice for a bit-for-bit comparison, and,
where the entry point accumulates, runs onto zeros (identical to the plain result) and onto a seeded base (the plain result
added within one rounding).  One case per kernel exceeds a single pass of its capped grid.  -s prints error / bound."""
import pytest
import torch

import spatial_ref as S

pytestmark = pytest.mark.gpu


def _ratio(tag, got, want, bound):
    """max |got - want| / bound; where the bound is zero the result has to be equal."""
    err = (got.double() - want).abs()
    z = bound <= 0
    assert bool((err[z] == 0).all()), tag
    r = float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0
    print(f"[{tag}] max error / bound = {r:.3f} over {got.numel()} elements")
    assert r <= 1.0, (tag, r)
    return r


def _one_rounding(tag, got, base, plain):
    """got = base + plain within ONE rounding: of the sum, or (when the compiler fuses the last product of `plain` into the
    sum) of the sum without plain's own rounding: |got - (base + plain)| <= u (|base + plain| + |plain|)."""
    s = base.double() + plain.double()
    assert bool(((got.double() - s).abs() <= S.U * (s.abs() + plain.double().abs())).all()), tag


def _src(t2d, ld, off, dev):
    """t2d [rows, C] placed as a column slice of a [rows, ld] sentinel matrix."""
    rows, C = t2d.shape
    _, v = S.strided(rows, C, ld, off, dev, fill=-S.SENTINEL)
    v.copy_(t2d)
    return v


def _twice(tag, make, run, intact):
    """run(view) on two fresh (buffer, view) pairs: bit-identical buffers, guard bands intact; returns the view."""
    out = []
    for _ in range(2):
        buf, v = make()
        run(v)
        out.append((buf, v))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]), f"{tag}: two runs differ"
    assert intact(out[0][0]), f"{tag}: wrote outside its destination"
    return out[0][1]


def _strided_dst(rows, C, ld, off, dev, init=None):
    def make():
        buf, v = S.strided(rows, C, ld, off, dev)
        if init is not None:
            v.copy_(init)
        return buf, v
    return make, (lambda buf: S.gaps_intact(buf, rows, C, ld, off))


def _flat_dst(n, dev, guard=S.AGUARD, init=None, dtype=torch.float32, fill=S.SENTINEL):
    def make():
        buf, v = S.guarded(n, dtype=dtype, device=dev, fill=fill, guard=guard)
        if init is not None:
            v.copy_(init.reshape(-1))
        return buf, v
    return make, (lambda buf: S.guard_intact(buf, n, fill=fill, guard=guard))


# ------------------------------------------------------------------------------------------------ 1. bilinear, channels-last
@pytest.mark.parametrize("case", S.NHWC_CASES + [S.NHWC_BIG_FWD], ids=lambda c: c[0])
def test_bilinear_nhwc_fwd(dev, case):
    """svl_bilinear_nhwc_fwd: both corner conventions at integer and fractional ratios, up and down, 1 x 1 broadcast, a single
    output row / column under align_corners (scale 0), rep in {1, 2, 3, 5}; plain, accumulate onto zeros and onto a base."""
    from semivl_amd import ops
    name, imgs, (h, w), (H, W), C, align, rep = case
    x, _, by, _ = [t.to(dev) for t in S.nhwc_inputs(case)]
    ldx, ldy, rows = C + 4, C + 12, imgs * rep * H * W
    xs = _src(x.view(-1, C), ldx, 4, dev)
    want, bound = S.bilinear_fwd_ref(x, H, W, align, rep)

    def run(acc):
        return lambda v: ops.bilinear_nhwc_fwd(xs, ldx, imgs, h, w, C, align, rep, H, W, v, ldy, accumulate=acc)
    mk, ok = _strided_dst(rows, C, ldy, 8, dev)
    plain = _twice(name, mk, run(False), ok)
    _ratio(f"bilinear_nhwc_fwd {name}", plain.reshape(want.shape), want, bound)
    mk, ok = _strided_dst(rows, C, ldy, 8, dev, init=torch.zeros(rows, C, device=dev))
    assert torch.equal(_twice(name + " +0", mk, run(True), ok), plain), f"{name}: accumulate onto zeros"
    mk, ok = _strided_dst(rows, C, ldy, 8, dev, init=by.view(rows, C))
    got = _twice(name + " +base", mk, run(True), ok)
    _one_rounding(name, got, by.view(rows, C), plain)
    wa, ba = S.bilinear_fwd_ref(x, H, W, align, rep, base=by)
    _ratio(f"bilinear_nhwc_fwd accumulate {name}", got.reshape(wa.shape), wa, ba)
    if name == S.NHWC_BIG_FWD[0]:
        assert rows * (C // 4) > S.one_pass()


@pytest.mark.parametrize("case,direct", [(c, d) for c in S.NHWC_CASES + [S.NHWC_BIG_BWD] for d in (False, True) if c[6] > 1 or not d],
                         ids=lambda v: v[0] if isinstance(v, tuple) else ("rep_in_kernel" if v else "through_ops"))
def test_bilinear_nhwc_bwd(dev, case, direct):
    """svl_bilinear_nhwc_bwd on a column slice of a wider gradient row (vlg_head.py's skip gradient), through
    ops.bilinear_nhwc_bwd (svl_sum_rep_f32 first, then rep = 1) and with the kernel's own rep loop."""
    from semivl_amd import ops
    name, imgs, (h, w), (H, W), C, align, rep = case
    _, dy, _, bx = [t.to(dev) for t in S.nhwc_inputs(case)]
    lddy, lddx, rows = C + 8, C + 4, imgs * h * w
    dys = _src(dy.view(-1, C), lddy, 4, dev)
    want, bound = S.bilinear_bwd_ref(dy, h, w, align, rep)

    def run(acc):
        return lambda v: ops.bilinear_nhwc_bwd(dys, lddy, imgs, h, w, C, align, rep, H, W, v, lddx, accumulate=acc,
                                               sum_first=not direct)
    mk, ok = _strided_dst(rows, C, lddx, 4, dev)
    plain = _twice(name, mk, run(False), ok)
    _ratio(f"bilinear_nhwc_bwd {name} {'direct' if direct else 'sum_rep'}", plain.reshape(want.shape), want, bound)
    mk, ok = _strided_dst(rows, C, lddx, 4, dev, init=torch.zeros(rows, C, device=dev))
    assert torch.equal(_twice(name + " +0", mk, run(True), ok), plain), f"{name}: accumulate onto zeros"
    mk, ok = _strided_dst(rows, C, lddx, 4, dev, init=bx.view(rows, C))
    got = _twice(name + " +base", mk, run(True), ok)
    _one_rounding(name, got, bx.view(rows, C), plain)
    if name == S.NHWC_BIG_BWD[0]:
        assert rows * (C // 4) > S.one_pass()


# ------------------------------------------------------------------------------------------------ 2. bilinear, planes
@pytest.mark.parametrize("case", S.PLANES_CASES + [S.PLANES_BIG_FWD, S.PLANES_BIG_BWD], ids=lambda c: c[0])
def test_bilinear_planes(dev, case):
    """svl_bilinear_planes_fwd on a 16-byte aligned destination (four columns per thread when W % 4 == 0) and on an unaligned
    one (scalar path), each under the bound and against each other; svl_bilinear_planes_bwd including ratios above 4.5 in x
    only (more contributing columns than its register window holds)."""
    from semivl_amd import ops
    name, planes, (h, w), (H, W), align = case
    x, dy = [t.to(dev) for t in S.planes_inputs(case)]
    want, bound = S.bilinear_fwd_ref(x[..., None], H, W, align)
    n = planes * H * W
    res = []
    for guard in (S.AGUARD, S.GUARD):
        mk, ok = _flat_dst(n, dev, guard=guard)
        res.append(_twice(f"{name} guard {guard}", mk, lambda v: ops.bilinear_planes_fwd(x, h, w, align, H, W, out=v.view(planes, H, W)), ok))
    _ratio(f"bilinear_planes_fwd {name} aligned", res[0].view(planes, H, W, 1), want, bound)
    _ratio(f"bilinear_planes_fwd {name} unaligned", res[1].view(planes, H, W, 1), want, bound)
    # the two paths are separate instantiations: the compiler may fuse multiply-adds (of the coordinate, of the interpolation)
    # differently, so each is an evaluation of its own under the same bound: they differ by at most twice that
    _ratio(f"bilinear_planes_fwd {name} vector vs scalar path", res[0].view(planes, H, W, 1), res[1].view(planes, H, W, 1).double(), 2 * bound)
    wantb, boundb = S.bilinear_bwd_ref(dy[..., None], h, w, align)
    mk, ok = _flat_dst(planes * h * w, dev, guard=S.GUARD)
    got = _twice(name + " bwd", mk, lambda v: ops.bilinear_planes_bwd(dy, h, w, align, H, W, out=v.view(planes, h, w)), ok)
    _ratio(f"bilinear_planes_bwd {name}", got.view(planes, h, w, 1), wantb, boundb)
    assert torch.equal(ops.bilinear_planes_bwd(dy, h, w, align, H, W).reshape(-1), got)
    if name == S.PLANES_BIG_FWD[0]:
        assert planes * H * (W // 4) > S.one_pass()
    if name == S.PLANES_BIG_BWD[0]:
        assert planes * h * w > S.one_pass()
    if name.startswith("fallback"):
        assert S._taps(S.axis_weights(w, W, align), S.axis_slack(w, W, align)) > 9 >= \
            S._taps(S.axis_weights(h, H, align), S.axis_slack(h, H, align))


# ------------------------------------------------------------------------------------------------ 3. sum_rep
@pytest.mark.parametrize("case", S.SUM_REP_CASES + [S.SUM_REP_BIG], ids=str)
def test_sum_rep(dev, case):
    """svl_sum_rep_f32 directly: rep in {1, 2, 3, 8, 21} (odd counts leave the unpaired tail), rows `ld` apart; rep <= 2 is
    one correctly rounded addition: bit-equal."""
    from semivl_amd import ops
    rep, groups, rows, C, ld, off = case
    src = S._rand((groups * rep, rows, C), 10 + rep).to(dev)
    ss = _src(src.view(-1, C), ld, off, dev)
    want, bound = S.sum_rep_ref(src, rep)
    mk, ok = _flat_dst(groups * rows * C, dev)
    got = _twice(f"sum_rep {case}", mk, lambda v: ops.sum_rep(ss, ld, groups, rep, rows, C, out=v.view(groups * rows, C)), ok)
    if rep <= 2:
        assert torch.equal(got.view(want.shape), want.float())
    else:
        _ratio(f"sum_rep {case}", got.view(want.shape), want, bound)
    if case == S.SUM_REP_BIG:
        assert groups * rows * (C // 4) > S.one_pass()


# ------------------------------------------------------------------------------------------------ 4. average pool + concat
@pytest.mark.parametrize("case", S.POOL_CASES + [S.POOL_BIG], ids=lambda c: c[0])
def test_avgpool_cat(dev, case):
    """svl_avgpool_cat_fwd / _bwd / _bwd_text: PH != PW, floor windows with different remainders on the two axes, the global
    pool without text, the scalar kernels (C or Ct not a multiple of 4), Ct in {2, 4, 64, 128, 256} for the text gradient."""
    from semivl_amd import ops
    name, imgs, (H, W), C, (PH, PW), Ct, nclass = case
    x, text, dy, base = [t.to(dev) if t is not None else None for t in S.pool_inputs(case)]
    Hp, Wp = H // PH, W // PW
    assert PH != PW and H != W and (Hp * PH == H or (H % PH != W % PW))
    want, bound = S.avgpool_cat_fwd_ref(x, PH, PW, text, nclass)
    mk, ok = _flat_dst(want.numel(), dev)
    y = _twice(name, mk, lambda v: ops.avgpool_cat_fwd(x.view(-1, C), imgs, H, W, C, (PH, PW), text, nclass,
                                                       out=v.view(-1, C + Ct)), ok)
    _ratio(f"avgpool_cat_fwd {name}", y.view(want.shape), want, bound)              # the text columns: bound 0 = equal
    wb, bb = S.avgpool_cat_bwd_ref(dy, H, W, C, PH, PW)
    n = imgs * H * W * C
    dtext = []
    mk, ok = _flat_dst(n, dev)

    def bwd(v):
        mt, okt = _flat_dst(max(nclass * Ct, 1), dev)
        tb, tv = mt()
        _, dt = ops.avgpool_cat_bwd(dy.view(-1, C + Ct), imgs, H, W, C, (PH, PW), Ct, nclass, out=v.view(-1, C),
                                    text_out=tv.view(nclass, Ct) if Ct else None)
        torch.cuda.synchronize()
        assert okt(tb)
        dtext.append(dt)
    plain = _twice(name + " bwd", mk, bwd, ok)
    _ratio(f"avgpool_cat_bwd {name}", plain.view(wb.shape), wb, bb)
    if Ct:
        wt, bt = S.avgpool_text_bwd_ref(dy, C, nclass)
        assert torch.equal(dtext[0], dtext[1])
        _ratio(f"avgpool_cat_bwd_text {name}", dtext[0], wt, bt)
    else:
        assert dtext[0] is None

    def acc(v):
        ops.avgpool_cat_bwd(dy.view(-1, C + Ct), imgs, H, W, C, (PH, PW), Ct, nclass, add_to=v.view(-1, C))
    mk, ok = _flat_dst(n, dev, init=torch.zeros(n, device=dev))
    assert torch.equal(_twice(name + " +0", mk, acc, ok), plain)
    mk, ok = _flat_dst(n, dev, init=base)
    got = _twice(name + " +base", mk, acc, ok)
    _one_rounding(name, got, base.reshape(-1), plain)
    outside = torch.ones(imgs, H, W, C, dtype=torch.bool, device=dev)
    outside[:, :Hp * PH, :Wp * PW] = False
    assert torch.equal(got.view(imgs, H, W, C)[outside], base[outside]), f"{name}: pixels outside the floor region changed"
    assert float(plain.view(imgs, H, W, C)[outside].abs().sum()) == 0.0
    if name == S.POOL_BIG[0]:
        assert imgs * H * W * (C // 4) > S.one_pass()
    if C % 4 == 0 and Ct % 4 == 0:
        # the same call on destinations that are not 16-byte aligned: the entry points then take their scalar kernels
        mk, ok = _flat_dst(want.numel(), dev, guard=S.GUARD)
        yu = _twice(name + " unaligned", mk, lambda v: ops.avgpool_cat_fwd(x.view(-1, C), imgs, H, W, C, (PH, PW), text, nclass,
                                                                         out=v.view(-1, C + Ct)), ok)
        assert yu.data_ptr() % 16 != 0
        _ratio(f"avgpool_cat_fwd {name} unaligned", yu.view(want.shape), want, bound)
        mk, ok = _flat_dst(n, dev, guard=S.GUARD)
        du = _twice(name + " bwd unaligned", mk, lambda v: ops.avgpool_cat_bwd(dy.view(-1, C + Ct), imgs, H, W, C, (PH, PW), Ct, nclass,
                                                                             out=v.view(-1, C)), ok)
        _ratio(f"avgpool_cat_bwd {name} unaligned", du.view(wb.shape), wb, bb)
        mk, ok = _flat_dst(n, dev, guard=S.GUARD, init=base)
        ga = _twice(name + " +base unaligned", mk, acc, ok)
        _one_rounding(name, ga, base.reshape(-1), du)
        assert torch.equal(ga.view(imgs, H, W, C)[outside], base[outside])


def test_avgpool_cat_refusals(dev):
    """Ct = 96 (256 % Ct != 0) and imgs % nclass != 0 are refused by svl_avgpool_cat_bwd_text: SVL_ERR_INVALID_ARG."""
    from semivl_amd import ops
    dy = torch.zeros(6 * 2 * 3, 8 + 96, device=dev)
    with pytest.raises(RuntimeError, match=r"status -1"):
        ops.avgpool_cat_bwd(dy, 6, 4, 9, 8, (2, 3), 96, 3)
    dy = torch.zeros(5 * 2 * 3, 8 + 64, device=dev)
    with pytest.raises(RuntimeError, match=r"status -1"):
        ops.avgpool_cat_bwd(dy, 5, 4, 9, 8, (2, 3), 64, 3)
    with pytest.raises(RuntimeError, match=r"status -1"):
        ops.avgpool_cat_fwd(torch.zeros(5 * 4 * 9, 8, device=dev), 5, 4, 9, 8, (5, 3), None, 1)      # PH > H
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. Conv2d(C -> 1)
@pytest.mark.parametrize("case", S.COUT1_CASES + S.WGRAD_EXTRA + [S.COUT1_BIG], ids=lambda c: c[0])
def test_conv_cout1(dev, case):
    """svl_conv_cout1_fwd (the LDS-tiled kernel at ragged H % 8, W % 32, C in {16, 32, 64}, with and without gn_in; the generic
    kernel with dilation, 5 x 3 and 7 x 7 taps, H < 8, beyond one pass of its grid) and svl_conv_cout1_wgrad on every 3 x 3
    case (maps smaller than a block's pixel lanes; block boundaries inside images), the input a column slice."""
    from semivl_amd import ops
    name, imgs, (H, W), C, (KH, KW), dil, pad, gn, ld, off = case
    x, wf, bias, gn_in, dy = [t.to(dev) if t is not None else None for t in S.cout1_inputs(case)]
    xs = _src(x.view(-1, C), ld, off, dev) if ld > C else x.view(-1, C)
    xop = S.gn_operand(x, gn_in) if gn else x.double()
    npix = imgs * H * W
    if not gn or ops.conv_cout1_gn_ok(H, W, C, KH, KW, dil, pad):
        want, bound = S.conv_cout1_fwd_ref(xop, wf, bias, KH, KW, dil, pad, gn)
        mk, ok = _flat_dst(npix, dev, guard=S.GUARD)
        y = _twice(name, mk, lambda v: ops.conv_cout1_fwd(xs, ld, imgs, H, W, C, wf, KH, KW, dil, pad, bias=bias,
                                                          out=v.view(npix, 1), gn_in=gn_in), ok)
        _ratio(f"conv_cout1_fwd {name}", y.view(want.shape), want, bound)
        nob = ops.conv_cout1_fwd(xs, ld, imgs, H, W, C, wf, KH, KW, dil, pad, gn_in=gn_in)
        wn, bn = S.conv_cout1_fwd_ref(xop, wf, None, KH, KW, dil, pad, gn)
        _ratio(f"conv_cout1_fwd no bias {name}", nob.view(wn.shape), wn, bn)
    if (KH, KW) == (3, 3):
        wg, bg = S.conv_cout1_wgrad_ref(dy, xop, dil, pad)
        mk, ok = _flat_dst(9 * C, dev, guard=S.GUARD)
        got = _twice(name + " wgrad", mk, lambda v: ops.conv_cout1_wgrad(dy.view(-1, 1), xs, ld, imgs, H, W, C, dil, pad,
                                                                        gn_in=gn_in, out=v.view(1, 9 * C)), ok)
        _ratio(f"conv_cout1_wgrad {name}", got, wg, bg)
    if name == S.COUT1_BIG[0]:
        assert npix > S.THIN_GRID_CAP * (256 // (C // 4))
    if name.startswith("tiny_map"):
        assert H * W < 256 // (C // 4)
    if name.startswith("block_edges"):
        nb = S.wgrad_chain(imgs, H, W, C)[1]
        assert nb > 1 and ((npix + nb - 1) // nb) % (H * W) != 0


def test_conv_cout1_gn_in_needs_the_tiled_form(dev):
    """gn_in with a geometry the tiled forward does not take is refused, not ignored."""
    from semivl_amd import ops
    x, wf, gn = torch.zeros(2 * 5 * 20, 32, device=dev), torch.zeros(9 * 32, device=dev), torch.zeros(2, 2, 32, device=dev)
    with pytest.raises(RuntimeError, match=r"status -1"):
        ops.conv_cout1_fwd(x, 32, 2, 5, 20, 32, wf, 3, 3, 1, 1, gn_in=gn)
    with pytest.raises(RuntimeError, match=r"status -1"):
        ops.conv_cout1_fwd(torch.zeros(2 * 9 * 20, 32, device=dev), 32, 2, 9, 20, 32, wf, 3, 3, 2, 2, gn_in=gn)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. tap_gather
@pytest.mark.parametrize("case", S.TAP_CASES + [S.TAP_BIG], ids=lambda c: c[0])
def test_tap_gather(dev, case):
    """svl_tap_gather: sign = +-1, KH != KW, dil in {1, 2}, pad != dil (K - 1) / 2, non-square."""
    from semivl_amd import ops
    name, imgs, (H, W), (KH, KW), dil, pad, sign = case
    T = S.tap_inputs(case).to(dev)
    want, bound = S.tap_gather_ref(T, KH, KW, dil, pad, sign)
    npix = imgs * H * W
    mk, ok = _flat_dst(npix, dev, guard=S.GUARD)
    got = _twice(name, mk, lambda v: ops.tap_gather(T.view(npix, KH * KW), imgs, H, W, KH, KW, dil, pad, sign,
                                                    out=v.view(npix, 1)), ok)
    _ratio(f"tap_gather {name}", got.view(want.shape), want, bound)
    if name == S.TAP_BIG[0]:
        assert npix > S.one_pass(S.THIN_GRID_CAP)


# ------------------------------------------------------------------------------------------------ 7. max pool
@pytest.mark.parametrize("case", S.MAXPOOL_CASES + [S.MAXPOOL_BIG], ids=lambda c: c[0])
def test_maxpool3x3s2(dev, case):
    """svl_maxpool3x3s2_fwd: values AND idx equal to the restatement (winning tap 0..8, first maximum in scan order, ties
    included, a constant plane: the first tap inside the image); svl_maxpool3x3s2_bwd from that idx."""
    from semivl_amd import ops
    name, imgs, (H, W), C, ties = case
    x, dy = [t.to(dev) for t in S.maxpool_inputs(case)]
    want, widx = S.maxpool_ref(x)
    Ho, Wo = want.shape[1], want.shape[2]
    n = want.numel()
    ibufs = []

    def fwd(v):
        ib, iv = S.guarded(n, dtype=torch.uint8, device=dev, fill=77, guard=S.AGUARD)
        _, idx, ho, wo = ops.maxpool3x3s2_fwd(x.view(-1, C), imgs, H, W, C, out=v.view(-1, C), idx_out=iv.view(-1, C))
        assert (ho, wo) == (Ho, Wo) and idx.data_ptr() == iv.data_ptr()
        ibufs.append(ib)
    mk, ok = _flat_dst(n, dev)
    y = _twice(name, mk, fwd, ok)
    assert torch.equal(ibufs[0], ibufs[1]) and S.guard_intact(ibufs[0], n, fill=77, guard=S.AGUARD)
    idx = ibufs[0][S.AGUARD:S.AGUARD + n].view(want.shape)
    assert torch.equal(y.view(want.shape), want), name
    assert torch.equal(idx, widx), f"{name}: {int((idx != widx).sum())} winners differ"
    wb, bb = S.maxpool_bwd_ref(dy, widx, H, W)
    mk, ok = _flat_dst(imgs * H * W * C, dev)
    dx = _twice(name + " bwd", mk, lambda v: ops.maxpool3x3s2_bwd(dy.view(-1, C), idx.reshape(-1, C), imgs, H, W, C,
                                                                  out=v.view(-1, C)), ok)
    _ratio(f"maxpool3x3s2_bwd {name}", dx.view(wb.shape), wb, bb)
    if name == S.MAXPOOL_BIG[0]:
        assert n // 4 > S.one_pass()
