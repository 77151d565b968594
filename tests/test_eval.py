"""Evaluation path: oracle vs the reference-captured fixture on CPU; product (HIP) vs the fixture on GPU."""
import os

import numpy as np
import pytest
import torch

from golden_util import assert_labels

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture():
    z = np.load(os.path.join(HERE, "golden", "eval_zegclip.npz"))
    g = torch.Generator().manual_seed(77)
    img = torch.randn(2, 3, 600, 700, generator=g)
    img = torch.nn.functional.avg_pool2d(img, 9, stride=1, padding=4)
    chk = np.array([img.double().sum().item(), img.double().abs().sum().item()])
    assert np.allclose(chk, z["img_checksum"], rtol=0, atol=1e-6), "seeded image stream differs from the fixture's"
    return z, img


def test_oracle_eval_matches_reference_fixture():
    from oracle import eval_oracle as E
    z, img = fixture()
    K, crop, stride = [int(v) for v in z["cfg"]]
    mask = torch.from_numpy(z["mask"]).long()
    with torch.no_grad():
        pred, final = E.predict_zegclip_sliding_window(E.ToyModel(K), img, mask.shape[-2:], crop, stride, K)
    assert np.array_equal(pred.numpy().astype(np.uint8), z["pred"])
    assert np.abs(final[:, :, ::8, ::8].numpy() - z["final_s8"]).max() < 1e-6
    i, u, t = E.intersection_and_union(pred.numpy(), mask.numpy(), K, 255)
    assert np.array_equal(i, z["inter"]) and np.array_equal(u, z["union"]) and np.array_equal(t, z["target"])
    with torch.no_grad():
        p_sw, f_sw = E.predict_sliding_window(E.ToyModel(K), img, crop, K)
        p_pd, f_pd = E.predict_padded_sliding_window(E.ToyModel(K), img, crop, stride, K)
    assert np.array_equal(p_sw.numpy().astype(np.uint8), z["pred_sw"])
    assert np.array_equal(p_pd.numpy().astype(np.uint8), z["pred_pd"])
    assert np.abs(f_sw[:, :, ::8, ::8].numpy() - z["final_sw_s8"]).max() < 1e-6


@pytest.mark.gpu
def test_hip_eval_matches_reference_fixture(dev):
    from oracle import eval_oracle as E
    from semivl_amd import ops
    from semivl_amd.evaluate import evaluate, intersection_and_union, predict
    z, img = fixture()
    K, crop, stride = [int(v) for v in z["cfg"]]
    cfg = dict(crop_size=crop, stride=stride, nclass=K)
    mask = torch.from_numpy(z["mask"]).long()
    w = E.ToyModel(K).w.data.to(dev).contiguous()

    class HipToy:  # same toy segmentor through the HIP GEMM: logits[b, n, p] = sum_k w[n, k] img[b, k, p]
        def eval(self):
            return self

        def __call__(self, x):
            b, c, h, ww = x.shape
            out = ops.empty(b, K, h, ww, device=x.device)
            ops.gemm(ops.A_MC, ops.B_KC, h * ww, K, c, ops.Op(x.contiguous(), h * ww, 0, c * h * ww, 0), ops.Op(w, c), out,
                     ldc_m=1, ldc_n=h * ww, batch=b, c_bso=K * h * ww)
            return out

    model = HipToy()
    with torch.no_grad():
        pred, final = predict(model, img.to(dev), mask.to(dev), "zegclip_sliding_window", cfg, return_logits=True)
    assert np.abs(final[:, :, ::8, ::8].cpu().numpy() - z["final_s8"]).max() < 1e-4
    # bit-exact prediction map; a flip is tolerated only where the reference's own top-2 logit gap is an fp tie
    with torch.no_grad():
        _, ofinal = E.predict_zegclip_sliding_window(E.ToyModel(K), img, mask.shape[-2:], crop, stride, K)
    t2 = ofinal.topk(2, dim=1).values
    tie = ((t2[:, 0] - t2[:, 1]) < 1e-6).numpy()
    hip_pred = pred.cpu().numpy().astype(np.uint8)
    flips = assert_labels(hip_pred, z["pred"], tie, "zegclip_sliding_window prediction")
    # integer confusion counts: bit-exact given the same prediction map
    i, u, t = intersection_and_union(torch.from_numpy(z["pred"]).long().to(dev), mask.to(dev), K, 255)
    assert np.array_equal(i.cpu().numpy(), z["inter"]) and np.array_equal(u.cpu().numpy(), z["union"])
    assert np.array_equal(t.cpu().numpy(), z["target"])
    # evaluate(): deferred single reduction == reference formula
    miou, iou = evaluate(model, [(img[:1], mask[:1], None), (img[1:], mask[1:], None)], "zegclip_sliding_window", cfg)
    # the metric is a pure function of the integer counts: it must match the reference formula on the SAME prediction to
    # rounding, and the fixture's mIoU itself whenever the prediction map is identical (no tie flips)
    hi, hu, _ = E.intersection_and_union(hip_pred, mask.numpy(), K, 255)
    assert abs(miou - E.miou(hi.astype(float), hu.astype(float))[0]) < 1e-9
    ref_miou, _ = E.miou(z["inter"].astype(float), z["union"].astype(float))
    assert flips > 0 or abs(miou - ref_miou) < 1e-9
    for mode, pk, fk in (("sliding_window", "pred_sw", "final_sw_s8"), ("padded_sliding_window", "pred_pd", "final_pd_s8")):
        with torch.no_grad():
            p_, f_ = predict(model, img.to(dev), mask.to(dev), mode, cfg, return_logits=True)
        assert np.abs(f_[:, :, ::8, ::8].cpu().numpy() - z[fk]).max() < 1e-5, mode
        assert (p_.cpu().numpy().astype(np.uint8) != z[pk]).mean() < 1e-5, mode   # (probability-averaged windows)


# ------------------------------------------------------------------------------------------------ through the real model
def vlm_fixture():
    import ast
    sys_path = os.path.join(HERE, "golden")
    z = np.load(os.path.join(sys_path, "eval_vlm.npz"))
    c = ast.literal_eval(str(z["cfg"]))
    g = torch.Generator().manual_seed(c["seed"])
    img = torch.randn(2, 3, c["H"], c["W"], generator=g)
    img = torch.nn.functional.avg_pool2d(img, 9, stride=1, padding=4)
    img = img / img.std()
    chk = np.array([img.double().sum().item(), img.double().abs().sum().item()])
    assert np.allclose(chk, z["img_checksum"], rtol=0, atol=1e-6), "seeded image stream differs from the fixture's"
    return z, c, img, torch.from_numpy(z["mask"]).long()


MODES = ("sliding_window", "zegclip_sliding_window", "original")


def test_oracle_eval_through_vlm_matches_reference_fixture(request):
    """The oracle VLM under the oracle `predict` restatements == the reference's VLM under the reference's `predict` on a
    160x150 image (windows of 128x128, 128x65, 75x128, 75x65 pixels; whole-image mode)."""
    from golden_util import build_oracle, fixture_state
    from oracle import eval_oracle as E
    z, c, img, mask = vlm_fixture()
    # (restored afterwards: later tests size their own thread pools from torch.get_num_threads())
    request.addfinalizer(lambda n=torch.get_num_threads(): torch.set_num_threads(n))
    torch.set_num_threads(8)
    orc = build_oracle(c)
    orc.load_state_dict(fixture_state(z, c, orc), strict=True)
    orc.eval()
    with torch.no_grad():
        res = dict(sliding_window=E.predict_sliding_window(orc, img, c["S"], 21),
                   zegclip_sliding_window=E.predict_zegclip_sliding_window(orc, img, mask.shape[-2:], c["S"], c["stride"], 21))
        fo = orc(img)
        res["original"] = (fo.argmax(dim=1), fo)
    for mode in MODES:
        pred, final = res[mode]
        assert np.array_equal(pred.numpy().astype(np.uint8), z[f"pred/{mode}"]), mode
        assert np.abs(final[:, :, ::4, ::4].numpy() - z[f"final_s4/{mode}"]).max() < 1e-5, mode
        i, u, t = E.intersection_and_union(pred.numpy(), mask.numpy(), 21, 255)
        assert np.array_equal(i, z[f"inter/{mode}"]) and np.array_equal(u, z[f"union/{mode}"]), mode


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_hip_evaluate_through_vlm_matches_reference_fixture(dev, mode):
    """semivl_amd.evaluate.predict / evaluate driving the PRODUCT VLM on windows that are not img_size: off-size and
    non-square token grids (8x5, 5x8, 5x5, 10x10 patches vs the 8x8 trained grid), per-forward pos-embed resize, the
    two chained output resizes (vlg_head.py:247, builder.py:93-97)."""
    from golden_util import build_hip, fixture_state
    from oracle import eval_oracle as E
    from semivl_amd.evaluate import evaluate, predict
    z, c, img, mask = vlm_fixture()
    hip = build_hip(c)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    hip.to(dev).eval()
    cfg = dict(crop_size=c["S"], stride=c["stride"], nclass=21)
    with torch.no_grad():   # one image at a time, exactly as evaluate() feeds the model (rounding depends on the batch shape)
        outs = [predict(hip, img[i:i + 1].to(dev), mask[i:i + 1].to(dev), mode, cfg, return_logits=True) for i in range(2)]
    pred, final = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    ref = z[f"final_s4/{mode}"]
    err = np.abs(final[:, :, ::4, ::4].cpu().numpy() - ref).max()
    # logits within north_star's 1e-3; summed window probabilities within the error a 1e-3 logit perturbation can cause
    # (|d softmax| <= |d logit| / 2 per window, <= 4 windows per pixel; measured 5e-5 on these 150x-gain logits)
    assert err < (1e-3 if mode != "sliding_window" else 2e-4), err
    hp = pred.cpu().numpy().astype(np.uint8)
    # bit-exact prediction map; a flip needs the reference's own top-2 gap at that pixel to be below the error measured in
    # this very run (x4: the error is measured on a 1/16 subsample of the map)
    tie = z[f"gap/{mode}"] <= max(1e-6, 4.0 * err)
    flips = assert_labels(hp, z[f"pred/{mode}"], tie, mode)
    assert flips <= 1e-4 * hp.size, flips
    print(f"[{mode}] max logit err {err:.2e}, label flips at ties {flips}")
    miou, _ = evaluate(hip, [(img[:1], mask[:1], None), (img[1:], mask[1:], None)], mode, cfg)
    hi, hu, _ = E.intersection_and_union(hp, mask.numpy(), 21, 255)
    assert abs(miou - E.miou(hi.astype(float), hu.astype(float))[0]) < 1e-9
    if flips == 0:
        assert abs(miou - E.miou(z[f"inter/{mode}"].astype(float), z[f"union/{mode}"].astype(float))[0]) < 1e-9
