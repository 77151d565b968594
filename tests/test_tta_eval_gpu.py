"""GPU: multi-scale + flip test-time augmentation of semivl_amd.evaluate.predict / evaluate.  The orchestration is checked
without a tolerance of its own: every view is rebuilt with ops.tta_view and sent through the (deterministic) single-view
`predict`, whose fp32 `final` is the one the TTA path saw; those are accumulated in float64 by tests/tta_ref.accum_ref, and
the returned mean scores must lie within the sum of the per-view bounds derived there.  Labels equal the float64 argmax except
where its top-2 gap is below twice that bound."""
import numpy as np
import pytest
import torch

import tta_ref as R

pytestmark = pytest.mark.gpu


def _hip_toy(dev):
    """tests/test_eval.py's toy segmentor through the HIP GEMM: logits[b, n, p] = sum_k w[n, k] img[b, k, p]."""
    from oracle import eval_oracle as E
    from semivl_amd import ops
    K = R.EVAL_K
    w = E.ToyModel(K).w.data.to(dev).contiguous()

    class HipToy:
        def eval(self):
            return self

        def __call__(self, x):
            b, c, h, ww = x.shape
            out = ops.empty(b, K, h, ww, device=x.device)
            ops.gemm(ops.A_MC, ops.B_KC, h * ww, K, c, ops.Op(x.contiguous(), h * ww, 0, c * h * ww, 0), ops.Op(w, c), out,
                     ldc_m=1, ldc_n=h * ww, batch=b, c_bso=K * h * ww)
            return out

    return HipToy()


def _check_tta(model, img, mask, mode, cfg, tta, tag):
    """predict(..., tta=tta) against the float64 accumulation of the rebuilt views' single-view `final`s; returns pred."""
    from semivl_amd import ops
    from semivl_amd.evaluate import predict
    h, w = img.shape[-2:]
    H, W = mask.shape[-2:]
    align = getattr(model, "align_corners", False)
    with torch.no_grad():
        pred, acc = predict(model, img, mask, mode, cfg, return_logits=True, tta=tta)
        assert acc.shape == (img.shape[0], cfg["nclass"], H, W) and pred.shape == (img.shape[0], H, W)
        views = R.tta_views(tta["ratios"], tta["flip"])
        want, bound = None, 0.0
        for r, f in views:
            view = ops.tta_view(img, int(h * r + 0.5), int(w * r + 0.5), f)
            assert view.shape[-2:] == (int(h * r + 0.5), int(w * r + 0.5))
            _, final = predict(model, view, mask, mode, cfg, return_logits=True)
            want, b = R.accum_ref(final, want, H, W, R.KIND[mode], align, f, 1.0 / len(views))
            bound = bound + b
    assert bool(torch.isfinite(bound).all()), tag
    err = (acc.double() - want).abs()
    ratio = (err / bound).max().item()
    t2 = want.topk(2, dim=1).values
    tie = (t2[:, 0] - t2[:, 1]) < 2 * bound.max(dim=1).values
    flips = pred != want.argmax(dim=1)
    print(f"[{tag}] {len(views)} views: max error / bound = {ratio:.3f}, labels differing at ties {int(flips.sum())} of {int(tie.sum())} ties")
    assert ratio <= 1.0, (tag, ratio)
    assert bool((want.sum(1) - 1).abs().max() < 1e-6), tag          # a mean of per-pixel distributions (n fl32(1 / n) is 1 to 2^-24)
    assert not bool((flips & ~tie).any()), (tag, int((flips & ~tie).sum()))
    return pred


@pytest.mark.parametrize("mode", R.EVAL_MODES)
def test_predict_tta_is_the_float64_mean_of_its_views(dev, mode):
    img, mask = R.eval_image().to(dev), R.eval_mask().to(dev)
    _check_tta(_hip_toy(dev), img, mask, mode, R.EVAL_CFG, R.EVAL_TTA, mode)


def test_predict_without_tta_is_the_single_view_body(dev):
    from semivl_amd import ops
    from semivl_amd.evaluate import _view_scores, predict
    model, img, mask = _hip_toy(dev), R.eval_image().to(dev), R.eval_mask().to(dev)
    with torch.no_grad():
        for mode in R.EVAL_MODES + ("center_crop",):
            for kw in ({}, dict(tta=None)):
                pred, final = predict(model, img, mask, mode, R.EVAL_CFG, return_logits=True, **kw)
                want = _view_scores(model, img, mask.shape[-2:], mode, R.EVAL_CFG)
                assert torch.equal(final, want), mode
                assert torch.equal(pred, ops.softmax_max(want.contiguous())[1]), mode
                assert torch.equal(pred, predict(model, img, mask, mode, R.EVAL_CFG, **kw)), mode
        with pytest.raises(ValueError, match="center_crop"):
            predict(model, img, mask, "center_crop", R.EVAL_CFG, tta=R.EVAL_TTA)
        with pytest.raises(ValueError):
            predict(model, img, mask, "original", R.EVAL_CFG, tta=dict(ratios=[]))


@pytest.mark.parametrize("mode", ("original", "padded_sliding_window"))
def test_evaluate_with_tta(dev, mode):
    """tta= and cfg['eval_tta'] give the same mIoU: the reference formula on the TTA prediction map."""
    from oracle import eval_oracle as E
    from semivl_amd.evaluate import evaluate, predict
    model, img, mask = _hip_toy(dev), R.eval_image(), R.eval_mask()
    loader = [(img[:1], mask[:1], None), (img[1:], mask[1:], None)]
    tta = dict(ratios=[0.5, 1.0], flip=True)
    m1, iou1 = evaluate(model, loader, mode, R.EVAL_CFG, tta=tta)
    m2, iou2 = evaluate(model, loader, mode, dict(R.EVAL_CFG, eval_tta=dict(img_ratios=(0.5, 1.0), flip=True)))
    assert m1 == m2 and np.array_equal(iou1, iou2)
    with torch.no_grad():
        pred = torch.cat([predict(model, i.to(dev), m.to(dev), mode, R.EVAL_CFG, tta=tta) for i, m, _ in loader])
    hi, hu, _ = E.intersection_and_union(pred.cpu().numpy(), mask.numpy(), R.EVAL_K, 255)
    assert abs(m1 - E.miou(hi.astype(float), hu.astype(float))[0]) < 1e-9
    assert 0.0 < m1 <= 100.0


@pytest.mark.parametrize("mode,ratios", (("original", (0.75, 1.0)), ("sliding_window", (0.5, 1.0))))
def test_predict_tta_through_the_product_model(dev, mode, ratios):
    """The product VLM (tests/golden/eval_vlm.npz state) on a 160 x 150 image, two ratios + flip, the model's own align_corners
    in the resize to the mask size.  'original': ratios (0.75, 1.0), views of 120 x 113 and 160 x 150 pixels.
    'sliding_window' (windows of 128, step 85): the 120 x 113 view would end in windows of 35 rows / 28 columns, fewer than the
    4 x 4 patches of 16 pixels the head's 4 x 4 pooling needs (the reference's AvgPool2d refuses them as well), so its downscaled
    view is the 80 x 75 one of ratio 0.5: one window of 5 x 4 patches."""
    from golden_util import build_hip, fixture_state
    from test_eval import vlm_fixture
    z, c, img, mask = vlm_fixture()
    hip = build_hip(c)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    hip.to(dev).eval()
    cfg = dict(crop_size=c["S"], stride=c["stride"], nclass=21)
    _check_tta(hip, img[:1].to(dev), mask[:1].to(dev), mode, cfg, dict(ratios=ratios, flip=True), f"vlm/{mode}")
