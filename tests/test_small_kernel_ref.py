"""CPU: the restatements of tests/small_kernel_ref.py against independent expressions (slicing, permute, the oracle, the
plain-C backend of the ABI), and the derived bounds against a plain fp32 torch evaluation on the very inputs the GPU file
(tests/test_small_kernels_gpu.py) uses -- so a GPU failure is a finding about the kernel, not about the checker."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cabi_cpu as K
import small_kernel_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ copy2d
@pytest.mark.parametrize("form", R.copy2d_forms(), ids=lambda f: f[0])
def test_copy2d_index_formula_is_the_slicing_expression(form):
    name, sshape, dshape, init, desc, acc, expr = form
    src = _rand(sshape, 11).double()
    dst = _rand(dshape, 12).double() if init is None else torch.full(dshape, float(init), dtype=torch.float64)
    s_off, sgrp, sgo, sld, d_off, dgrp, dgo, dld, rows, C = desc
    got = R.copy2d_ref(src, s_off, sgrp, sgo, sld, dst, d_off, dgrp, dgo, dld, rows, C, acc).view(dshape)
    assert torch.equal(got, expr(src, dst)), name
    # destination rows are distinct (the contract the header states)
    di = R.copy2d_indices(d_off, dgrp, dgo, dld, rows, C)
    assert di.unique().numel() == di.numel(), name


def test_copy2d_forms_cover_every_call_site():
    """Thirteen call sites in vit.py / evaluate.py (the one at vit.py:686 in both of its accumulate settings)."""
    import re
    n = 0
    for f in ("model/vit.py", "evaluate.py"):
        n += len(re.findall(r"ops\.copy2d\(", open(os.path.join(os.path.dirname(HERE), "semivl_amd", f)).read()))
    names = {f[0].split("_")[0] for f in R.copy2d_forms()}
    assert n == 13 and len(names) == 13, (n, sorted(names))


@pytest.mark.parametrize("case", R.copy2d_generic_cases(), ids=lambda c: c[0])
def test_copy2d_generic_descriptors_against_a_python_loop(case):
    name, ns, nd, desc, acc = case
    s_off, sgrp, sgo, sld, d_off, dgrp, dgo, dld, rows, C = desc
    src, dst = _rand((ns,), 21).double(), _rand((nd,), 22).double()
    exp = dst.clone()
    for i in range(rows):
        for c in range(C):
            v = src[s_off + (i // sgrp) * sgo + (i % sgrp) * sld + c]
            j = d_off + (i // dgrp) * dgo + (i % dgrp) * dld + c
            exp[j] = exp[j] + v if acc else v
    assert torch.equal(R.copy2d_ref(src, s_off, sgrp, sgo, sld, dst, d_off, dgrp, dgo, dld, rows, C, acc), exp)


def test_copy2d_wrapper_refuses_overlapping_accumulation():
    """ops.copy2d checks the distinct-destination rule host side, before any library call."""
    from semivl_amd import ops
    t = torch.zeros(64)
    with pytest.raises(AssertionError):
        ops.copy2d(t, 0, 2, 0, 4, t, 0, 2, 0, 4, 4, 4, accumulate=True)      # dst_go = 0 with rows > dgrp
    with pytest.raises(AssertionError):
        ops.copy2d(t, 0, 2, 8, 4, t, 0, 2, 8, 0, 4, 4, accumulate=True)      # dst_ld = 0 with dgrp > 1


# ------------------------------------------------------------------------------------------------ permute4
@pytest.mark.parametrize("shape", R.CONV_SHAPES, ids=str)
def test_conv_pack_tuples_are_the_permutes(shape):
    Co, Ci, kh, kw = shape
    w = _rand(shape, 31)
    t = R.conv_pack_tuples(*shape)
    wf = R.permute4_ref(w, *t["fwd"][:2])
    assert torch.equal(wf, t["fwd"][2](w).contiguous())
    assert torch.equal(R.permute4_ref(w, *t["dgrad"][:2]), t["dgrad"][2](w).contiguous())
    back = R.permute4_ref(wf.view(Co, kh * kw * Ci), *t["unpack"][:2])
    assert torch.equal(back, t["unpack"][2](wf).contiguous()) and torch.equal(back, w)


@pytest.mark.parametrize("shape", R.CONVT_SHAPES, ids=str)
def test_convt_pack_tuples_are_the_permutes(shape):
    Cin, Cu = shape
    w = _rand((Cin, Cu, 2, 2), 32)
    t = R.convt_pack_tuples(Cin, Cu)
    for k in ("fwd", "bwd"):
        assert torch.equal(R.permute4_ref(w, *t[k][:2]), t[k][2](w).contiguous()), k
    wb = R.permute4_ref(w, *t["bwd"][:2]).view(Cin, 4 * Cu)             # [Cin, (a, b, co)]: the weight gradient's layout
    assert torch.equal(R.permute4_ref(wb, *t["wgrad"][:2]), w)
    assert torch.equal(R.permute4_ref(wb, *t["wgrad"][:2]), t["wgrad"][2](wb).contiguous())


def test_pack_tuples_are_the_ones_the_product_builds():
    """ops.pack_conv_w / ops.unpack_conv_wgrad (CPU path of ops.permute4) give what the restated tuples give."""
    from semivl_amd import ops
    for shape in R.CONV_SHAPES:
        w = _rand(shape, 33)
        t = R.conv_pack_tuples(*shape)
        wf, wd = ops.pack_conv_w(w)
        assert torch.equal(wf.view(t["fwd"][0]), R.permute4_ref(w, *t["fwd"][:2]))
        assert torch.equal(wd.view(t["dgrad"][0]), R.permute4_ref(w, *t["dgrad"][:2]))
        assert torch.equal(ops.unpack_conv_wgrad(wf, *shape), w)


# ------------------------------------------------------------------------------------------------ reduce_slabs
def test_reduce_slabs_ref_and_the_cancellation_case():
    g = torch.Generator().manual_seed(41)
    slabs = torch.randn(9, 1001, generator=g)
    out = torch.randn(1001, generator=g)
    assert torch.equal(R.reduce_slabs_ref(out, slabs, False), slabs.double().sum(0).float())
    acc = R.reduce_slabs_ref(out, slabs, True)
    assert (acc.double() - (out.double() + slabs.double().sum(0))).abs().max() <= 2.0 ** -24 * 16
    n = 64
    s = R.cancellation_slabs(n, 5)
    assert torch.equal(R.reduce_slabs_ref(torch.zeros(5), s, False), torch.full((5,), float(n - 2)))
    chain = torch.zeros(5)
    for k in range(n):
        chain = chain + s[k]
    assert torch.equal(chain, torch.zeros(5)), "an fp32 chain visibly fails on this input"


# ------------------------------------------------------------------------------------------------ affine / softmax bounds
@pytest.mark.parametrize("case", R.affine_cases(), ids=lambda c: c[0])
def test_affine_bound_holds_for_plain_fp32(case):
    name, x, k4 = case
    k = k4[:, None, :, None, None]
    y32 = ((x * k[0] + k[1]) - k[2]) / k[3]
    ratio = ((y32.double() - R.affine_ref(x, k4)).abs() / R.affine_bound(x, k4)).max().item()
    print(f"affine {name}: fp32 torch error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert x.shape[0] > 1 and x[0, 0].numel() % 2 == 1
    assert len({tuple(k4[:, c].tolist()) for c in range(k4.shape[1])}) == k4.shape[1], "distinct constants per channel"


def test_affine_constants_are_builders():
    src = open(os.path.join(os.path.dirname(HERE), "semivl_amd", "model", "builder.py")).read()
    for row in R.CLIP_K4:
        assert str(row) in src, row


@pytest.mark.parametrize("case", R.softmax_cases(), ids=lambda c: c[0])
def test_softmax_bound_holds_for_plain_fp32(case):
    name, x = case
    N = x.shape[1]
    m = x.max(dim=1, keepdim=True).values
    e = torch.exp(x - m)
    p32 = e * (1.0 / e.sum(dim=1, keepdim=True))
    ratio = ((p32.double() - R.softmax_ref(x)).abs() / R.softmax_bound(x)).max().item()
    dsum = (p32.double().sum(1) - 1).abs().max().item()
    print(f"softmax {name}: fp32 torch error / bound = {ratio:.3f}, |plane sum - 1| / bound = {dsum / R.softmax_sum_bound(N):.3f}")
    assert ratio <= 1.0 and dsum <= R.softmax_sum_bound(N)


def test_case_sizes_reach_the_grid_stride_loop():
    assert max(c[1].numel() for c in R.affine_cases()) > R.one_pass(4)
    assert max(c[1].shape[0] * c[1][0, 0].numel() for c in R.softmax_cases()) > R.one_pass(1)
    assert {c[1].shape[1] for c in R.softmax_cases()} == {1, 19, 21, 150}
    big = [f for f in R.copy2d_forms() if f[4][8] * f[4][9] > R.one_pass(4)]
    assert big, "one copy2d form exceeds a pass of the capped grid"


# ------------------------------------------------------------------------------------------------ iou_hist
@pytest.mark.parametrize("Kc", [1, 19, 21, 256])
def test_iou_hist_ref_matches_oracle_and_c_backend(Kc):
    from oracle import eval_oracle as E
    g = torch.Generator().manual_seed(51 + Kc)
    n = 5003
    pred = torch.randint(0, Kc, (n,), generator=g)
    tgt = torch.randint(0, Kc, (n,), generator=g)
    pred[::7] = 255
    pred[3::11] = -1
    tgt[1::5] = 255
    tgt[2::13] = 254
    ref = R.iou_hist_ref(pred, tgt, Kc, 255).numpy()
    i, u, t = E.intersection_and_union(pred.numpy(), tgt.numpy(), Kc, 255)
    assert np.array_equal(ref[:Kc], i) and np.array_equal(ref[2 * Kc:], t) and np.array_equal(ref[Kc:2 * Kc], u - t + i)
    hist = np.zeros(3 * Kc, np.int64)
    K.check(K.load().svl_iou_hist_i64(K.ptr(pred.numpy()), K.ptr(tgt.numpy()), n, Kc, 255, K.ptr(hist), None))
    assert np.array_equal(hist, ref)
    if Kc < 254:
        assert ref[2 * Kc:].sum() == ((tgt >= 0) & (tgt < Kc)).sum().item(), "targets 254 / 255 are in no bin"


# ------------------------------------------------------------------------------------------------ conf_ratio / conf_avg
@pytest.mark.parametrize("B,HW", [(1, 1), (3, 10), (5, 1001)])
def test_conf_refs_match_oracle_expressions_and_c_backend(B, HW):
    lib = K.load()
    g = torch.Generator().manual_seed(61 + B)
    conf = (torch.randint(0, 21, (B, 1, HW), generator=g).float() / 20.0).contiguous()
    conf[:, :, 0] = torch.tensor(19.0) / 20.0                           # == fp32(0.95): exactly at the threshold, valid below
    ign = torch.zeros(B, 1, HW, dtype=torch.int64)
    ign[torch.rand(B, 1, HW, generator=g) < 0.3] = 255
    ign[:, :, 0] = 0
    for thresh in (0.95, 0.0):
        ref = R.conf_ratio_ref(conf, ign, thresh)
        v = ign != 255
        assert torch.equal(ref, (((conf >= thresh) & v).sum((1, 2)) / v.sum((1, 2))))          # train_utils.py:39-40
        ratio = np.zeros(B, np.float32)
        ws = np.zeros(int(lib.svl_conf_avg_ws_doubles(B)), np.float64)
        K.check(lib.svl_conf_ratio_f32(K.ptr(conf.numpy()), K.ptr(ign.numpy()), B, HW, thresh, K.ptr(ratio), K.ptr(ws), None))
        assert np.array_equal(ratio, ref.numpy())
    assert ((conf == torch.tensor(0.95)) & (ign != 255)).any(), "confidences sit exactly at the threshold"
    f = np.zeros(1, np.float64)
    ws = np.zeros(int(lib.svl_conf_avg_ws_doubles(B)), np.float64)
    K.check(lib.svl_conf_avg_factor(K.ptr(conf.numpy()), K.ptr(ign.numpy()), B, HW, K.ptr(f), K.ptr(ws), None))
    ref = R.conf_avg_factor_ref(conf, ign)
    assert abs(f[0] - ref) <= 1e-12 * abs(ref)
    v = (ign != 255)
    sp = dict(dim=(1, 2), keepdim=True)
    assert abs(((conf.double() * v).sum(**sp) / v.sum(**sp)).sum().item() - ref) <= 1e-12 * abs(ref)


# ------------------------------------------------------------------------------------------------ loss assembly
def test_loss_ref_matches_oracle_helpers():
    """loss_ref on the sums of a small case == the oracle's confidence_weighted_loss / compute_mc_loss assembled as
    semivl.py:317-321 does, for 'pixelwise' and 'pixelavg' and the three guidance normalisers."""
    from oracle import semivl_oracle as O
    g = torch.Generator().manual_seed(71)
    B, N, H, W = 2, 7, 12, 10
    logits = (torch.randn(B, N, H, W, generator=g) * 2).double()
    target = torch.randint(0, N, (B, H, W), generator=g)
    tx = target.clone()
    tx[torch.rand(B, H, W, generator=g) < 0.1] = 255
    conf = torch.rand(B, H, W, generator=g).double()
    ign = torch.zeros(B, H, W, dtype=torch.int64)
    ign[:, -3:] = 255
    mc = torch.randint(0, N, (B, H, W), generator=g)
    mc[torch.rand(B, H, W, generator=g) < 0.4] = 255
    lam, numel, valid = 0.07, float(B * H * W), ign != 255
    ce = F.cross_entropy(logits, target, reduction="none")
    ce_m = F.cross_entropy(logits, mc, ignore_index=255, reduction="none")
    lx = F.cross_entropy(logits, tx, ignore_index=255)
    for mode in ("pixelwise", "pixelavg"):
        for reduce in ("mean_all", "mean_valid", "mean"):
            lu = O.confidence_weighted_loss(ce, conf, ign, mode, 0.6)
            lmc = O.compute_mc_loss(logits, mc, ign, reduce)
            want = (lx + lu * 0.25 + lu * 0.25 + lu * 0.5) / 2.0 + lmc * 0.25 * lam + lmc * 0.25 * lam + lmc * 0.5 * lam
            w = ((conf >= 0.6) & valid).double() if mode == "pixelwise" else torch.ones_like(conf)
            row = [(w * ce).sum().item(), ce_m.sum().item(), (conf * valid).sum().item(), valid.sum().item()]
            sums = [[F.cross_entropy(logits, tx, ignore_index=255, reduction="sum").item(), 0.0, 0.0, (tx != 255).sum().item()],
                    row, row, row]
            fac = None if mode == "pixelwise" else [R.conf_avg_factor_ref(conf, ign)] * 3
            mcn = {"mean_all": None, "mean_valid": [valid.sum().item()] * 3, "mean": [(mc != 255).sum().item()] * 3}[reduce]
            out, _ = R.loss_ref(sums, numel, lam, fac, mcn)
            tol = 1e-12
            lam32 = float(np.float32(lam))
            want = want.item() + (lam32 - lam) * lmc.item()
            assert abs(out[0] - want) <= tol * abs(want), (mode, reduce, out[0], want)
            assert abs(out[1] - lx.item()) <= tol * lx.item() and abs(out[2] - lu.item()) <= tol * max(1.0, lu.item())
            assert abs(out[5] - lmc.item()) <= tol * lmc.item()


@pytest.mark.parametrize("case", R.loss_cases(), ids=lambda c: c[0])
def test_loss_and_gscale_refs_match_c_backend_and_each_other(case):
    name, counts, sums, numel, lam, factors, mc_counts = case
    lib = K.load()
    gs = np.zeros((4, 2), np.float32)
    K.check(lib.svl_semivl_gscale(K.ptr(counts), numel, lam, K.ptr(factors), K.ptr(mc_counts), K.ptr(gs), None))
    gref = R.gscale_ref(counts, numel, lam, factors, mc_counts)
    g32 = gref.astype(np.float32)
    assert (np.abs(gs.astype(np.float64) - g32) <= np.spacing(np.abs(g32))).all() and gs[0, 1] == 0
    out = np.zeros(8, np.float32)
    K.check(lib.svl_semivl_loss(K.ptr(sums), numel, lam, K.ptr(factors), K.ptr(mc_counts), K.ptr(out), None))
    ref, mag = R.loss_ref(sums, numel, lam, factors, mc_counts)
    assert (np.abs(out - ref) <= 8 * R.U * mag).all(), (out, ref)
    # the forward weights are the gradient weights: d loss / d sums[i][0] = g_t[i], d loss / d sums[i][1] = g_m[i]
    for i in range(4):
        for j in (0, 1):
            if gref[i, j] == 0.0:
                continue
            s2 = sums.copy()
            s2[i, j] += 1.0 / gref[i, j]
            assert abs((R.loss_ref(s2, numel, lam, factors, mc_counts)[0][0] - ref[0]) - 1.0) <= 1e-9, (i, j)
    assert counts.min() > 2 ** 24 or "above_2p24" not in name


# ------------------------------------------------------------------------------------------------ eltwise
def test_gelu_ref_and_c_backend_fill():
    x = _rand((4097,), 81)
    assert (R.gelu_ref(x) - F.gelu(x.double())).abs().max() < 1e-14
    buf, p = R.guarded(1001)
    K.check(K.load().svl_fill_f32(K.ptr(p.numpy()), 0.0, 1001, None))
    assert torch.equal(p, torch.zeros(1001)) and R.guard_intact(buf, 1001)


# ------------------------------------------------------------------------------------------------ predict edge geometries
def test_oracle_predict_matches_reference_on_edge_geometries():
    """oracle/eval_oracle.py's restatements of `predict` against the reference's own outputs (tests/golden/eval_edges.npz) on
    images smaller than the crop, a fractional stride, and (plain slicing) center_crop."""
    from oracle import eval_oracle as E
    z = np.load(os.path.join(HERE, "golden", "eval_edges.npz"))
    assert os.path.getsize(os.path.join(HERE, "golden", "eval_edges.npz")) <= os.path.getsize(
        os.path.join(HERE, "golden", "eval_zegclip.npz"))
    Kc, crop = R.EDGE_CFG["nclass"], R.EDGE_CFG["crop_size"]
    model = E.ToyModel(Kc)
    cases = R.edge_cases()
    assert len(cases) == 17
    for key, mode, cfg, (h, w), mask_hw in cases:
        img = R.edge_image(h, w)
        chk = np.array([img.double().sum().item(), img.double().abs().sum().item()])
        assert np.allclose(chk, z[f"{key}/img_checksum"], rtol=0, atol=1e-6), key
        assert f"{key}/raises" not in z.files, "the reference raises on none of these geometries"
        with torch.no_grad():
            if mode == "zegclip_sliding_window":
                pred, final = E.predict_zegclip_sliding_window(model, img, mask_hw, crop, cfg["stride"], Kc)
            elif mode == "sliding_window":
                pred, final = E.predict_sliding_window(model, img, crop, Kc)
            elif mode == "padded_sliding_window":
                pred, final = E.predict_padded_sliding_window(model, img, crop, cfg["stride"], Kc)
            else:
                sh, sw = (h - crop) // 2, (w - crop) // 2
                final = model(img[:, :, sh:sh + crop, sw:sw + crop])
                pred = final.argmax(dim=1)
        assert final.shape[-2:] == ((crop, crop) if mode == "center_crop" else tuple(mask_hw)), key
        assert np.array_equal(pred.numpy().astype(np.uint8), z[f"{key}/pred"]), key
        assert np.abs(final[:, :, ::4, ::4].numpy() - z[f"{key}/final_s4"]).max() < 1e-6, key
        t2 = final.topk(2, dim=1).values
        assert np.array_equal((t2[:, 0] - t2[:, 1]).clamp(max=R.EDGE_GAP_CLIP).numpy(), z[f"{key}/gap"]), key
