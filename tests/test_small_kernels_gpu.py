"""GPU: the small kernels between the large ones' results and a loss, a gradient scale, a weight gradient or an mIoU, each
through semivl_amd.ops against the plain restatements of tests/small_kernel_ref.py (ATen only as the checker):
svl_copy2d_f32, svl_permute4_f32, svl_reduce_slabs_f32, svl_affine_planes_f32, svl_softmax_planes_f32, svl_iou_hist_i64,
svl_conf_ratio_f32, svl_conf_avg_factor, svl_semivl_gscale, svl_semivl_loss, svl_eltwise_f32 modes 3-7, svl_fill_f32 /
ops.zeros, and evaluate.predict on geometries smaller than the crop.

Every kernel: one case beyond a single pass of the capped grid (R.one_pass), one on the scalar path where a vector path
exists, a sentinel guard band around every written buffer, two calls compared bit for bit."""
import os

import numpy as np
import pytest
import torch

import small_kernel_ref as R
from golden_util import assert_labels

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _rand(shape, seed, dev, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. copy2d
def _run_copy2d(dev, src, dshape, init, desc, acc, expr, name):
    from semivl_amd import ops
    s_off, sgrp, sgo, sld, d_off, dgrp, dgo, dld, rows, C = desc
    n = int(np.prod(dshape))
    buf0, pay0 = R.guarded(n, device=dev)
    pay0.copy_(_rand((n,), 7, dev) if init is None else torch.full((n,), float(init), device=dev))
    want = R.copy2d_ref(src.double(), s_off, sgrp, sgo, sld, buf0.double(), d_off + R.GUARD, dgrp, dgo, dld, rows, C, acc).float()
    bufs = []
    for _ in range(2):
        buf = buf0.clone()
        ops.copy2d(src, s_off, sgrp, sgo, sld, buf[R.GUARD:R.GUARD + n], d_off, dgrp, dgo, dld, rows, C, accumulate=acc)
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]), f"{name}: deterministic"
    assert torch.equal(bufs[0], want), f"{name}: index formula (guard band and untouched elements included)"
    assert R.guard_intact(bufs[0], n), name
    if expr is not None:   # the slicing expression in fp32: a plain copy is bit-equal to the source, accumulate to dst + src
        assert torch.equal(bufs[0][R.GUARD:R.GUARD + n].view(dshape), expr(src, pay0.view(dshape))), name


@pytest.mark.parametrize("form", R.copy2d_forms(), ids=lambda f: f[0])
def test_copy2d_call_forms(dev, form):
    """svl_copy2d_f32 in each of the thirteen call forms of vit.py / evaluate.py at ViT-B sizes (T = 1025, E = 768, B = 2) and
    the eval window sizes (crop 512 of 600 x 700, 21 classes; odd offsets and widths).  eval29_window_add (11 M elements)
    exceeds one pass of the grid."""
    name, sshape, dshape, init, desc, acc, expr = form
    _run_copy2d(dev, _rand(sshape, 3, dev), dshape, init, desc, acc, expr, name)


def test_copy2d_token_slice_beyond_one_grid_pass(dev):
    form = [f for f in R.copy2d_forms(B=6) if f[0] == "vit513_feat_tokens"][0]
    name, sshape, dshape, init, desc, acc, expr = form
    assert desc[8] * desc[9] > R.one_pass(4)
    _run_copy2d(dev, _rand(sshape, 4, dev), dshape, init, desc, acc, expr, name + "_B6")


@pytest.mark.parametrize("case", R.copy2d_generic_cases(), ids=lambda c: c[0])
def test_copy2d_broadcast_descriptors(dev, case):
    """src_ld = 0 / src_go = 0 (broadcast), C in {1, 3, 5, 768}, odd element offsets, plain and accumulating."""
    name, ns, nd, desc, acc = case
    _run_copy2d(dev, _rand((ns,), 5, dev), (nd,), None, desc, acc, None, name)


def test_copy2d_refuses_overlapping_accumulation(dev):
    from semivl_amd import ops
    t = torch.zeros(64, device=dev)
    with pytest.raises(AssertionError):
        ops.copy2d(t, 0, 2, 0, 4, t, 32, 2, 0, 4, 4, 4, accumulate=True)
    with pytest.raises(AssertionError):
        ops.copy2d(t, 0, 2, 8, 4, t, 32, 2, 8, 0, 4, 4, accumulate=True)
    ops.copy2d(t, 0, 2, 0, 4, t, 32, 2, 0, 4, 2, 4, accumulate=True)         # rows <= dgrp: distinct, accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. permute4
def _run_permute4(dev, src, shape, strides, name):
    from semivl_amd import ops
    n = int(np.prod(shape))
    want = R.permute4_ref(src, shape, strides)
    bufs = []
    for _ in range(2):
        buf, pay = R.guarded(n, device=dev)
        out = ops.permute4(src, shape, strides, out=pay.view(shape))
        assert out.data_ptr() == pay.data_ptr()
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]), name
    assert torch.equal(bufs[0][R.GUARD:R.GUARD + n].view(shape), want) and R.guard_intact(bufs[0], n), name
    assert torch.equal(ops.permute4(src, shape, strides), want), name
    return want


@pytest.mark.parametrize("shape", R.CONV_SHAPES, ids=str)
def test_permute4_conv_packs(dev, shape):
    """svl_permute4_f32 on every tuple ops.pack_conv_w / ops.unpack_conv_wgrad build, bit-equal to as_strided().contiguous();
    unpack(pack(w)) == w through the product's own functions; a source with a storage offset."""
    from semivl_amd import ops
    Co, Ci, kh, kw = shape
    w = _rand(shape, 11, dev)
    t = R.conv_pack_tuples(*shape)
    wf = _run_permute4(dev, w, *t["fwd"][:2], f"fwd{shape}")
    _run_permute4(dev, w, *t["dgrad"][:2], f"dgrad{shape}")
    back = _run_permute4(dev, wf.view(Co, kh * kw * Ci), *t["unpack"][:2], f"unpack{shape}")
    assert torch.equal(back, w)
    pf, pd = ops.pack_conv_w(w)
    assert torch.equal(pf.view(t["fwd"][0]), wf) and torch.equal(pd.view(t["dgrad"][0]), t["dgrad"][2](w).contiguous())
    assert torch.equal(ops.unpack_conv_wgrad(pf, *shape), w)
    store = torch.cat((torch.full((3,), R.SENTINEL, device=dev), w.reshape(-1)))
    off = store[3:].view(shape)
    assert off.storage_offset() == 3
    _run_permute4(dev, off, *t["fwd"][:2], f"fwd{shape}+3")


@pytest.mark.parametrize("shape", R.CONVT_SHAPES, ids=str)
def test_permute4_convtranspose_packs(dev, shape):
    """The three ConvTranspose2d(k 2, s 2) permutes of vlg_head.py (forward pack, weight-gradient unpack, backward pack)."""
    Cin, Cu = shape
    w = _rand((Cin, Cu, 2, 2), 12, dev)
    t = R.convt_pack_tuples(Cin, Cu)
    for k in ("fwd", "bwd"):
        got = _run_permute4(dev, w, *t[k][:2], f"convT {k}{shape}")
        assert torch.equal(got, t[k][2](w).contiguous())
    wb = R.permute4_ref(w, *t["bwd"][:2]).view(Cin, 4 * Cu)
    assert torch.equal(_run_permute4(dev, wb, *t["wgrad"][:2], f"convT wgrad{shape}"), w)


def test_permute4_beyond_one_grid_pass(dev):
    shape = (512, 1024, 3, 3)
    assert int(np.prod(shape)) > R.one_pass(4)
    t = R.conv_pack_tuples(*shape)
    _run_permute4(dev, _rand(shape, 13, dev), *t["fwd"][:2], "fwd big")


# ------------------------------------------------------------------------------------------------ 3. reduce_slabs
def _run_reduce(dev, slabs, acc, name):
    from semivl_amd import ops
    count = slabs.shape[1]
    init = _rand((count,), 22, dev)
    want = R.reduce_slabs_ref(init, slabs, acc)
    bufs = []
    for _ in range(2):
        buf, pay = R.guarded(count, device=dev)
        pay.copy_(init)
        ops.reduce_slabs(pay, slabs, accumulate=acc)
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]), name
    assert torch.equal(bufs[0][R.GUARD:R.GUARD + count], want) and R.guard_intact(bufs[0], count), name
    return bufs[0][R.GUARD:R.GUARD + count]


@pytest.mark.parametrize("nslab", [1, 7, 8, 9, 64, 500])
def test_reduce_slabs_is_an_ordered_double_sum(dev, nslab):
    """svl_reduce_slabs_f32: slabs added in index order in double (from `out` when accumulating), one rounding -- bit-equal to
    the Python loop; odd count (around the unroll-by-8 boundary in nslab)."""
    slabs = _rand((nslab, 10001), 21, dev)
    for acc in (False, True):
        _run_reduce(dev, slabs, acc, f"nslab {nslab} acc {acc}")


def test_reduce_slabs_beyond_one_grid_pass(dev):
    count = R.one_pass(1) + 77
    _run_reduce(dev, _rand((7, count), 23, dev), True, "grid stride")


@pytest.mark.parametrize("nslab", [9, 64, 500])
def test_reduce_slabs_keeps_what_an_fp32_chain_loses(dev, nslab):
    """2^25 + 1 + ... + 1 - 2^25: exactly nslab - 2 in double, 0 in an fp32 chain (the claim the full-size float64 gate of the
    weight gradients rests on)."""
    got = _run_reduce(dev, R.cancellation_slabs(nslab, 1001, dev), False, f"cancellation {nslab}")
    assert torch.equal(got, torch.full((1001,), float(nslab - 2), device=dev))


# ------------------------------------------------------------------------------------------------ 4. affine_planes
@pytest.mark.parametrize("case", R.affine_cases(), ids=lambda c: c[0])
def test_affine_planes_within_derived_bound(dev, case):
    """svl_affine_planes_f32 vs float64 under |y - y64| <= 4 u (|x k0| + |k1| + |k2|) / |k3| (R.affine_bound): the ImageNet ->
    CLIP constants of builder.py and four distinct random constants per channel; C = 3 and 5, odd HW, several images."""
    from semivl_amd import ops
    name, x, k4 = case
    x, k4 = x.to(dev), k4.to(dev).contiguous()
    n = x.numel()
    bufs = []
    for _ in range(2):
        buf, pay = R.guarded(n, device=dev)
        ops.affine_planes(x, k4, out=pay.view(x.shape))
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]) and R.guard_intact(bufs[0], n), name
    y = bufs[0][R.GUARD:R.GUARD + n].view(x.shape)
    ratio = ((y.double() - R.affine_ref(x, k4)).abs() / R.affine_bound(x, k4)).max().item()
    print(f"[affine_planes {name}] max error / bound = {ratio:.3f} over {n} elements")
    assert ratio <= 1.0, (name, ratio)
    assert torch.equal(ops.affine_planes(x, k4), y)


# ------------------------------------------------------------------------------------------------ 5. softmax_planes
@pytest.mark.parametrize("case", R.softmax_cases(), ids=lambda c: c[0])
def test_softmax_planes_within_derived_bound(dev, case):
    """svl_softmax_planes_f32 vs float64 softmax under |p - p64| <= 2 (|x_c - max| + N + 5) u p64 + 2^-126 and plane sums within
    (N + 4) u of 1 (R.softmax_bound): N in {1, 19, 21, 150}, spreads up to +-200, all-equal logits, odd HW."""
    from semivl_amd import ops
    name, x = case
    x = x.to(dev)
    n, N = x.numel(), x.shape[1]
    bufs = []
    for _ in range(2):
        buf, pay = R.guarded(n, device=dev)
        ops.softmax_planes(x, out=pay.view(x.shape))
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]) and R.guard_intact(bufs[0], n), name
    p = bufs[0][R.GUARD:R.GUARD + n].view(x.shape)
    ratio = ((p.double() - R.softmax_ref(x)).abs() / R.softmax_bound(x)).max().item()
    dsum = (p.double().sum(1) - 1).abs().max().item()
    print(f"[softmax_planes {name}] max error / bound = {ratio:.3f}, max |plane sum - 1| / bound = "
          f"{dsum / R.softmax_sum_bound(N):.3f}")
    assert ratio <= 1.0, (name, ratio)
    assert dsum <= R.softmax_sum_bound(N), (name, dsum)
    assert torch.equal(ops.softmax_planes(x), p)


# ------------------------------------------------------------------------------------------------ 6. iou_hist
def _hist(dev, pred, tgt, K, calls=1):
    from semivl_amd import ops
    buf, pay = R.guarded(3 * K, dtype=torch.int64, device=dev, fill=7)
    pay.zero_()
    for _ in range(calls):
        ops.iou_hist(pred, tgt, K, 255, pay)
    assert R.guard_intact(buf, 3 * K, fill=7)
    return pay.clone()


@pytest.mark.parametrize("K", [1, 19, 21, 150, 256, 4096])
def test_iou_hist_matches_bincount(dev, K):
    """svl_iou_hist_i64 == the int64 bincount restatement of intersectionAndUnion: predictions outside [0, K) (255, -1),
    targets 255 (ignored) and 254 (in no bin unless K > 254); two calls into one histogram give the sum."""
    g = torch.Generator().manual_seed(60 + K)
    n = 1_200_003                                       # odd, beyond the 2^20 threads of one grid pass
    pred = torch.randint(0, K, (n,), generator=g)
    tgt = torch.where(torch.rand(n, generator=g) < 0.6, pred, torch.randint(0, K, (n,), generator=g))
    pred[::7] = 255
    pred[3::11] = -1
    tgt[1::5] = 255
    tgt[2::13] = 254
    pred, tgt = pred.to(dev), tgt.to(dev)
    want = R.iou_hist_ref(pred, tgt, K, 255)
    h1, h1b = _hist(dev, pred, tgt, K), _hist(dev, pred, tgt, K)
    assert torch.equal(h1, h1b) and torch.equal(h1, want)
    assert torch.equal(_hist(dev, pred, tgt, K, calls=2), 2 * want)
    if K < 254:
        assert int(want[2 * K:].sum()) == int(((tgt >= 0) & (tgt < K)).sum())


def test_iou_hist_refuses_more_than_4096_classes(dev):
    from semivl_amd import ops
    z = torch.zeros(16, dtype=torch.int64, device=dev)
    hist = torch.zeros(3 * 4097, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match=r"status -1"):       # SVL_ERR_INVALID_ARG
        ops.iou_hist(z, z, 4097, 255, hist)
    assert int(hist.abs().sum()) == 0


def test_iou_hist_one_class_does_not_wrap(dev):
    """n = 1.25 * 2^24 + 3 pixels of ONE class: the worst case for the per-block 32-bit LDS counters."""
    n = int(2 ** 24 * 1.25) + 3
    pred = torch.full((n,), 3, dtype=torch.int64, device=dev)
    h = _hist(dev, pred, pred, 21)
    want = torch.zeros(63, dtype=torch.int64, device=dev)
    want[3] = want[21 + 3] = want[42 + 3] = n
    assert torch.equal(h, want) and torch.equal(h, R.iou_hist_ref(pred, pred, 21))
    assert torch.equal(h, _hist(dev, pred, pred, 21))


# ------------------------------------------------------------------------------------------------ 7. conf_ratio / conf_avg_factor
def _conf_case(dev, B, HW, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    conf = torch.randint(0, 21, (B, 1, HW), generator=g, device=dev).float() / 20.0      # 19 / 20 == fp32(0.95) exactly
    ign = torch.where(torch.rand(B, 1, HW, generator=g, device=dev) < 0.3, 255, 0)
    conf[:, :, 0] = torch.tensor(19.0) / 20.0
    ign[:, :, 0] = 0
    return conf.contiguous(), ign.contiguous()


def _ratio(dev, conf, ign, thresh):
    from semivl_amd import ops
    B = conf.shape[0]
    bufs = []
    for _ in range(2):
        buf, pay = R.guarded(B, device=dev)
        ops.conf_ratio(conf, ign, thresh, out=pay)
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]) or bool(torch.isnan(bufs[0]).any())
    assert R.guard_intact(bufs[0], B)
    return bufs[0][R.GUARD:R.GUARD + B].clone()


@pytest.mark.parametrize("HW", [1, 10, 512 * 512, 801 * 801])
@pytest.mark.parametrize("B", [1, 16, 65])
def test_conf_ratio_and_avg_factor(dev, B, HW):
    """svl_conf_ratio_f32 == fp32(#confident valid) / fp32(#valid) from integer sums, with confidences exactly at the threshold
    (>= counts them) and threshold 0; svl_conf_avg_factor within 1e-12 of the float64 expression of train_utils.py:43-46.
    B = 65 needs a second block of the final kernel; HW = 10 leaves most chunks empty."""
    from semivl_amd import ops
    conf, ign = _conf_case(dev, B, HW, 70 + B)
    for thresh in (0.95, 0.0):
        got, want = _ratio(dev, conf, ign, thresh), R.conf_ratio_ref(conf, ign, thresh)
        assert torch.equal(got, want), (thresh, (got - want).abs().max().item())
    at = ((conf == torch.tensor(19.0) / 20.0) & (ign != 255)).reshape(B, -1).sum(1)
    above = ((conf > torch.tensor(19.0) / 20.0) & (ign != 255)).reshape(B, -1).sum(1)
    assert bool((at > 0).all()), "every image has valid confidences exactly at the threshold"
    assert not torch.equal(R.conf_ratio_ref(conf, ign, 0.95), above.float() / (ign != 255).reshape(B, -1).sum(1).float())
    g = torch.Generator(device=dev).manual_seed(90 + B)
    cavg = torch.rand(B, 1, HW, generator=g, device=dev)
    vals = []
    for _ in range(2):
        buf, pay = R.guarded(1, dtype=torch.float64, device=dev)
        ops.conf_avg_factor(cavg, ign, pay)
        assert R.guard_intact(buf, 1)
        vals.append(pay.item())
    want = R.conf_avg_factor_ref(cavg, ign)
    print(f"[conf_avg_factor B={B} HW={HW}] relative error {abs(vals[0] - want) / abs(want):.2e}")
    assert vals[0] == vals[1] and abs(vals[0] - want) <= 1e-12 * abs(want)


def test_conf_ratio_image_without_valid_pixels(dev):
    """0 / 0 is NaN for that image, as torch's is; the other images' entries are unaffected."""
    conf, ign = _conf_case(dev, 16, 1001, 77)
    ign[5] = 255
    got, want = _ratio(dev, conf, ign, 0.95), R.conf_ratio_ref(conf, ign, 0.95)
    assert bool(torch.isnan(got[5])) and bool(torch.isnan(want[5]))
    keep = torch.arange(16, device=dev) != 5
    assert torch.equal(got[keep], want[keep]) and not bool(torch.isnan(got[keep]).any())


# ------------------------------------------------------------------------------------------------ 8. semivl_gscale / semivl_loss
def _loss_gpu(dev, sums, numel, lam, fac, mcn):
    from semivl_amd import ops
    outs = []
    for _ in range(2):
        buf, pay = R.guarded(8, device=dev)
        ops.semivl_loss(torch.from_numpy(sums).to(dev), numel, lam, pay, factors=fac, mc_counts=mcn)
        assert R.guard_intact(buf, 8)
        outs.append(pay.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


@pytest.mark.parametrize("case", R.loss_cases(), ids=lambda c: c[0])
def test_semivl_gscale_and_loss(dev, case):
    """svl_semivl_gscale within 1 fp32 ulp of the fp32 rounding of the double expression (gscale[1] == 0); svl_semivl_loss's
    eight outputs within 8 u sum|terms| of float64; factors x mc_counts in all four combinations, counts above 2^24, lam = 0.
    The two kernels agree: raising sums[i][0] (sums[i][1]) by delta moves the loss by g_t[i] delta (g_m[i] delta) to 1e-5
    relative.  delta makes the change 8: the forward bound above (8 u sum|terms| <= 2e-5 per evaluation on these cases, twice)
    then lies inside 1e-5 of the change, so the check cannot fail on rounding alone."""
    from semivl_amd import ops
    name, counts, sums, numel, lam, factors, mc_counts = case
    fac = None if factors is None else torch.from_numpy(factors).to(dev)
    mcn = None if mc_counts is None else torch.from_numpy(mc_counts).to(dev)
    gs = []
    for _ in range(2):
        buf, pay = R.guarded(8, device=dev)
        ops.semivl_gscale(torch.from_numpy(counts).to(dev), numel, lam, pay, factors=fac, mc_counts=mcn)
        assert R.guard_intact(buf, 8)
        gs.append(pay.cpu().numpy().reshape(4, 2))
    gref = R.gscale_ref(counts, numel, lam, factors, mc_counts)
    g32 = gref.astype(np.float32)
    assert np.array_equal(gs[0], gs[1]) and gs[0][0, 1] == 0.0
    assert (np.abs(gs[0].astype(np.float64) - g32.astype(np.float64)) <= _ulp32(g32)).all(), (gs[0], gref)
    out = _loss_gpu(dev, sums, numel, lam, fac, mcn)
    ref, mag = R.loss_ref(sums, numel, lam, factors, mc_counts)
    ratio = (np.abs(out.astype(np.float64) - ref) / (8 * R.U * mag + 1e-300)).max()
    print(f"[semivl_loss {name}] max error / bound = {ratio:.3f}; loss {out[0]:.6f}")
    assert ratio <= 1.0, (out, ref)
    assert np.array_equal(sums[:, 3], counts.astype(np.float64))
    change = 8.0
    assert 2 * 8 * R.U * (mag[0] + change) <= 1e-5 * change
    for i in range(4):
        for j in (0, 1):
            g = float(gs[0][i, j])
            if g == 0.0:
                continue
            s2 = sums.copy()
            s2[i, j] += change / g
            moved = float(_loss_gpu(dev, s2, numel, lam, fac, mcn)[0]) - float(out[0])
            assert abs(moved - change) <= 1e-5 * change, (name, i, j, moved)


# ------------------------------------------------------------------------------------------------ 9. eltwise 3-7, fill, zeros
def _eltwise_inputs(dev, n, aligned):
    """a, b (b away from zero) and a guarded output; aligned: 16 B aligned pointers (vector path when n % 4 == 0), else every
    pointer one element past alignment (a view) -- the scalar path whatever n is."""
    sh = 0 if aligned else 1
    a = _rand((n + sh,), 31, dev)[sh:]
    b = _rand((n + sh,), 32, dev)[sh:]
    b = torch.where(b >= 0, b + 0.5, b - 0.5)
    if not aligned:
        b = torch.cat((b.new_zeros(1), b))[1:]
    guard = 64 if aligned else R.GUARD
    assert (a.data_ptr() % 16 == 0) == aligned and (b.data_ptr() % 16 == 0) == aligned
    return a, b, guard


@pytest.mark.parametrize("n,aligned", [(4096, True), (4 * (R.one_pass(4) + 256), True), (1001, False), (4096, False),
                                       (R.one_pass(4) + 77, False)])
def test_eltwise_modes_3_to_7(dev, n, aligned):
    """svl_eltwise_f32: 3 (a b), 4 (copy), 6 (relu), 7 (a / b: the window-count division of zegclip_sliding_window) bit-equal to
    torch fp32 (no fast-math flag: the division is correctly rounded); 5 within 1e-6 of the float64 erf GELU.  Vector path
    (n % 4 == 0, aligned) and scalar path (odd n, or pointers offset by one element), each beyond one grid pass once."""
    from semivl_amd import ops
    a, b, guard = _eltwise_inputs(dev, n, aligned)
    want = {3: a * b, 4: a.clone(), 6: torch.relu(a), 7: a / b}
    for mode in (3, 4, 5, 6, 7):
        bufs = []
        for _ in range(2):
            buf, pay = R.guarded(n, device=dev, guard=guard)
            assert (pay.data_ptr() % 16 == 0) == aligned
            ops.eltwise(mode, a, b if mode in (3, 7) else None, out=pay)
            bufs.append(buf)
        assert torch.equal(bufs[0], bufs[1]) and R.guard_intact(bufs[0], n, guard=guard), mode
        got = bufs[0][guard:guard + n]
        if mode == 5:
            err = (got.double() - R.gelu_ref(a)).abs().max().item()
            print(f"[eltwise gelu n={n} aligned={aligned}] max |error| vs float64 {err:.2e}")
            assert err < 1e-6
        else:
            assert torch.equal(got, want[mode]), mode


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64])
def test_fill_and_zeros_on_integer_types(dev, dtype):
    """svl_fill_f32 through ops.fill (guard band) and ops.zeros (exact zeros for fp32 / int32 / int64 with odd element counts,
    over memory that held other values a moment ago; the integer types are filled through an fp32 view)."""
    from semivl_amd import ops
    per = 4 // torch.empty((), dtype=dtype).element_size() if dtype != torch.int64 else 0.5
    for n in (1, 1001, int((R.one_pass(4) + 77) * per) | 1):
        dirty = torch.full((n,), 13, dtype=dtype, device=dev)
        del dirty                                           # the caching allocator hands this block to the next request
        z = ops.zeros(n, dtype=dtype, device=dev)
        z2 = ops.zeros(n, dtype=dtype, device=dev)
        assert z.dtype == dtype and z.shape == (n,) and torch.equal(z, z2)
        assert int((z != 0).sum()) == 0, (dtype, n)
        words = n * z.element_size() // 4
        buf, pay = R.guarded(words, device=dev)
        ops.fill(pay, 0.0)
        assert R.guard_intact(buf, words) and int((pay.view(torch.int32) != 0).sum()) == 0
        ops.fill(pay, -2.5)
        assert R.guard_intact(buf, words) and torch.equal(pay, torch.full((words,), -2.5, device=dev))
    assert n * z.element_size() // 4 > R.one_pass(4)


# ------------------------------------------------------------------------------------------------ 10. predict on edge geometries
def _hip_toy(dev, K):
    from oracle import eval_oracle as E
    from semivl_amd import ops
    w = E.ToyModel(K).w.data.to(dev).contiguous()

    class HipToy:  # the toy segmentor of tests/test_eval.py through the HIP GEMM: logits[b, n, p] = sum_k w[n, k] img[b, k, p]
        def eval(self):
            return self

        def __call__(self, x):
            b, c, h, ww = x.shape
            out = ops.empty(b, K, h, ww, device=x.device)
            ops.gemm(ops.A_MC, ops.B_KC, h * ww, K, c, ops.Op(x.contiguous(), h * ww, 0, c * h * ww, 0), ops.Op(w, c), out,
                     ldc_m=1, ldc_n=h * ww, batch=b, c_bso=K * h * ww)
            return out
    return HipToy()


@pytest.mark.parametrize("case", R.edge_cases(), ids=lambda c: c[0])
def test_predict_edge_geometries_match_reference_fixture(dev, case):
    """semivl_amd.evaluate.predict against the reference's own `predict` (tests/golden/eval_edges.npz): images smaller than
    the crop in one or both dimensions, exactly the crop, one pixel more; zegclip with the final align-corners resize;
    padded windows with an integer and a fractional stride; center_crop.  `final` within the tolerances of
    test_hip_eval_matches_reference_fixture (1e-4 on logits, 1e-5 on summed probabilities); labels bit-exact except where the
    reference's top-2 gap is below twice that tolerance (two maps that close can order the two classes either way)."""
    from semivl_amd.evaluate import predict
    key, mode, cfg, (h, w), mask_hw = case
    z = np.load(os.path.join(HERE, "golden", "eval_edges.npz"))
    img = R.edge_image(h, w)
    chk = np.array([img.double().sum().item(), img.double().abs().sum().item()])
    assert np.allclose(chk, z[f"{key}/img_checksum"], rtol=0, atol=1e-6), "seeded image stream differs from the fixture's"
    model = _hip_toy(dev, cfg["nclass"])
    mask = torch.zeros(2, *mask_hw, dtype=torch.long, device=dev)
    if f"{key}/raises" in z.files:                          # (none today: the reference accepts every geometry listed)
        with pytest.raises(Exception):
            predict(model, img.to(dev), mask, mode, cfg, return_logits=True)
        return
    with torch.no_grad():
        pred, final = predict(model, img.to(dev), mask, mode, cfg, return_logits=True)
        pred2, final2 = predict(model, img.to(dev), mask, mode, cfg, return_logits=True)
    assert torch.equal(pred, pred2) and torch.equal(final, final2)
    tol = 1e-4 if mode in ("zegclip_sliding_window", "center_crop") else 1e-5
    ref = z[f"{key}/final_s4"]
    got = final[:, :, ::4, ::4].cpu().numpy()
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    err = np.abs(got - ref).max()
    flips = assert_labels(pred.cpu().numpy().astype(np.uint8), z[f"{key}/pred"], z[f"{key}/gap"] <= 2 * tol, key)
    print(f"[predict {key}] final {tuple(final.shape)} max error {err:.2e} (tolerance {tol:.0e}), label flips at ties {flips}")
    assert err < tol, (key, err)
