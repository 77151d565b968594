"""Golden vectors for the evaluation path, captured from the reference's OWN `predict` / `intersectionAndUnion`
(build container only; needs /root/reference).  Writes tests/golden/eval_zegclip.npz; `gen_golden_eval.py edges` writes
tests/golden/eval_edges.npz instead: `predict` on images smaller than the crop, a fractional stride and center_crop."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def edges(ref_predict):
    """The reference's `predict` with ToyModel on the geometries of tests/small_kernel_ref.py::edge_cases: per case the
    prediction map, min(top-2 gap of `final`, EDGE_GAP_CLIP) and `final` subsampled by 4 -- or, if the reference itself
    raises there, the exception's type name under '<key>/raises'."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import small_kernel_ref as R
    from oracle import eval_oracle as E
    torch.Tensor.cuda = lambda self, *a, **k: self      # the probability-averaging modes call .cuda() on fresh tensors
    model = E.ToyModel(R.EDGE_CFG["nclass"])
    out = {}
    for key, mode, cfg, (h, w), mask_hw in R.edge_cases():
        img = R.edge_image(h, w)
        out[f"{key}/img_checksum"] = np.array([img.double().sum().item(), img.double().abs().sum().item()])
        mask = torch.zeros(2, *mask_hw, dtype=torch.long)
        try:
            with torch.no_grad():
                pred, final = ref_predict(model, img, mask, mode, cfg, return_logits=True)
        except Exception as e:  # noqa: BLE001 -- recorded: the product must raise there too
            out[f"{key}/raises"] = np.array(type(e).__name__)
            print(f"{key}: the reference raises {type(e).__name__}: {e}")
            continue
        t2 = final.topk(2, dim=1).values if final.shape[1] > 1 else None
        gap = (t2[:, 0] - t2[:, 1]).clamp(max=R.EDGE_GAP_CLIP)
        out[f"{key}/pred"] = pred.numpy().astype(np.uint8)
        out[f"{key}/gap"] = gap.numpy().astype(np.float32)
        out[f"{key}/final_s4"] = final[:, :, ::4, ::4].numpy()
        print(f"{key}: final {tuple(final.shape)}, near-ties {(gap < 1e-5).sum().item()}")
    path = os.path.join(HERE, "eval_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote eval_edges.npz", os.path.getsize(path) / 1e6, "MB")


def main():
    os.chdir(REF)
    sys.path.insert(0, REF)
    import _ref_shim
    _ref_shim.install()
    from third_party.unimatch.supervised import predict as ref_predict
    if sys.argv[1:] == ["edges"]:
        return edges(ref_predict)
    from third_party.unimatch.util.utils import intersectionAndUnion as ref_iau
    from oracle import eval_oracle as E
    K, crop, stride = 21, 512, 426
    cfg = dict(crop_size=crop, stride=stride, nclass=K)
    g = torch.Generator().manual_seed(77)
    img = torch.randn(2, 3, 600, 700, generator=g)
    # smooth the image a little so that argmax regions are not pure noise
    img = torch.nn.functional.avg_pool2d(img, 9, stride=1, padding=4)
    mask = torch.randint(0, K, (2, 75, 88), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :590, :690]
    mask[torch.rand(mask.shape, generator=g) < 0.03] = 255
    model = E.ToyModel(K)
    with torch.no_grad():
        pred, final = ref_predict(model, img, mask, "zegclip_sliding_window", cfg, return_logits=True)
        opred, ofinal = E.predict_zegclip_sliding_window(model, img, mask.shape[-2:], crop, stride, K)
    assert torch.equal(pred, opred) and torch.equal(final, ofinal), "oracle restatement differs from the reference"
    # the probability-averaging modes call .cuda() on fresh tensors: run them on the CPU by neutralising it
    torch.Tensor.cuda = lambda self, *a, **k: self
    sw_mask = mask[:, :, :] if False else torch.zeros(2, 600, 700, dtype=torch.long)
    with torch.no_grad():
        p_sw, f_sw = ref_predict(model, img, sw_mask, "sliding_window", cfg, return_logits=True)
        p_pd, f_pd = ref_predict(model, img, sw_mask, "padded_sliding_window", cfg, return_logits=True)
        o_sw = E.predict_sliding_window(model, img, crop, K)
        o_pd = E.predict_padded_sliding_window(model, img, crop, stride, K)
    assert torch.equal(p_sw, o_sw[0]) and torch.equal(f_sw, o_sw[1]) and torch.equal(p_pd, o_pd[0]) and torch.equal(f_pd, o_pd[1])
    print("sliding_window / padded_sliding_window: reference == oracle")
    ri = ref_iau(pred.numpy(), mask.numpy(), K, 255)
    oi = E.intersection_and_union(pred.numpy(), mask.numpy(), K, 255)
    assert all(np.array_equal(a, b) for a, b in zip(ri, oi))
    print("reference == oracle: pred maps identical, counts identical; mIoU", E.miou(ri[0].astype(float), ri[1].astype(float))[0])
    np.savez_compressed(os.path.join(HERE, "eval_zegclip.npz"), img_checksum=np.array([img.double().sum().item(), img.double().abs().sum().item()]),
                        mask=mask.numpy().astype(np.uint8), pred=pred.numpy().astype(np.uint8),
                        final_s8=final[:, :, ::8, ::8].numpy(), inter=ri[0], union=ri[1], target=ri[2],
                        pred_sw=p_sw.numpy().astype(np.uint8), final_sw_s8=f_sw[:, :, ::8, ::8].numpy(),
                        pred_pd=p_pd.numpy().astype(np.uint8), final_pd_s8=f_pd[:, :, ::8, ::8].numpy(),
                        cfg=np.array([K, crop, stride]))
    print("wrote eval_zegclip.npz", os.path.getsize(os.path.join(HERE, "eval_zegclip.npz")) / 1e6, "MB")


if __name__ == "__main__":
    main()
