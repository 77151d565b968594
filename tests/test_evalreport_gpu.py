"""GPU: semivl_amd.report.evaluate_report, its file export, data.ValLoader and `python -m semivl_amd.tools.eval`.  The table is
held to tests/evalreport_ref.py's restatement on `predict`'s own labels (exact), `miou` / `iou_class` to `evaluate` on the
same loader (bit for bit), the written PNGs and .pt files to `predict`'s labels and `final` (exact), with the toy segmentor
and the tiny product VLM of tests/test_tta_eval_gpu.py."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import evalreport_ref as R
import tta_ref as T

pytestmark = pytest.mark.gpu
FULL = dict(metrics=["mIoU", "mAcc", "mDice", "mFscore"], beta=1, nan_to_num=None)


@pytest.fixture(scope="module")
def toy(dev):
    from test_tta_eval_gpu import _hip_toy
    img, mask = T.eval_image((2, 3, 75, 90)), T.eval_mask(hw=(75, 90))
    mask[0, 10:14, 5:40] = 254
    return _hip_toy(dev), img, mask, dict(T.EVAL_CFG), {True: dict(ratios=(0.5, 1.0), flip=True), False: None}


@pytest.fixture(scope="module")
def vlm(dev):
    """The product VLM (tests/golden/eval_vlm.npz state) on its 160 x 150 images; windows of 128, step 85."""
    from golden_util import build_hip, fixture_state
    from test_eval import vlm_fixture
    z, c, img, mask = vlm_fixture()
    hip = build_hip(c)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    hip.to(dev).eval()
    cfg = dict(crop_size=c["S"], stride=c["stride"], nclass=21)
    tta = {"original": dict(ratios=(0.75, 1.0), flip=True), "sliding_window": dict(ratios=(0.5, 1.0), flip=True)}
    return hip, img, mask, cfg, tta


def _loader(img, mask, ids=(None, None)):
    return [(img[:1], mask[:1], ids[0]), (img[1:], mask[1:], ids[1])]


def _check_report(dev, model, img, mask, cfg, mode, tta):
    from semivl_amd.evaluate import evaluate, predict
    from semivl_amd.report import evaluate_report
    K = cfg["nclass"]
    cfg = dict(cfg, eval_report=FULL)
    loader = _loader(img, mask)
    rep = evaluate_report(model, loader, mode, cfg, tta=tta)
    with torch.no_grad():
        pred = torch.cat([predict(model, i.to(dev), m.to(dev), mode, cfg, tta=tta) for i, m, _ in loader])
    want = R.confusion_ref(pred, mask.to(dev), K)
    assert np.array_equal(rep.table.reshape(-1), want.cpu().numpy())
    assert int(rep.table.sum()) == int((mask != 255).sum()) and int(rep.table[:K, :K].sum()) > 0
    m, iou = evaluate(model, loader, mode, cfg, tta=tta)
    assert rep.miou == m and np.array_equal(rep.iou_class, iou)
    # evaluate itself is unchanged: the reference's formula on the restated rows
    inter, parea, tarea = (v.cpu().numpy().astype(np.float64) for v in R.derived_rows(want, K))
    ref_iou = inter / (parea + tarea - inter + 1e-10) * 100.0
    assert np.array_equal(iou, ref_iou) and m == float(np.mean(ref_iou)) and 0.0 < m <= 100.0
    got, ref = rep.metrics(), R.metrics_ref(*R.derived_rows(rep.table, K), FULL["metrics"], 1)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert np.allclose(got[k], ref[k], rtol=0, atol=1e-12, equal_nan=True), k
    # cfg['eval_tta'] is picked up like evaluate does
    if tta is not None:
        rep2 = evaluate_report(model, loader, mode, dict(cfg, eval_tta=tta))
        assert np.array_equal(rep2.table, rep.table)
    return rep


@pytest.mark.parametrize("with_tta", [False, True])
@pytest.mark.parametrize("mode", ["original", "sliding_window"])
def test_report_through_the_toy_segmentor(dev, toy, mode, with_tta):
    model, img, mask, cfg, tta = toy
    rep = _check_report(dev, model, img, mask, cfg, mode, tta[with_tta])
    assert int(rep.table[cfg["nclass"]].sum()) == int((mask == 254).sum())          # 254: the extra row, not ignored


@pytest.mark.parametrize("with_tta", [False, True])
@pytest.mark.parametrize("mode", ["original", "sliding_window"])
def test_report_through_the_product_model(dev, vlm, mode, with_tta):
    model, img, mask, cfg, tta = vlm
    _check_report(dev, model, img, mask, cfg, mode, tta[mode] if with_tta else None)


def _read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "P", im.mode
        return np.array(im), im.getpalette()


@pytest.mark.parametrize("palette", [None, [7, 8, 9, 250, 0, 1, 2, 3, 4, 5, 6, 7, 255, 255, 0]])
def test_export_writes_predictions_and_logits(dev, toy, tmp_path, palette):
    """Batches of one (ids as a str, as the loader yields them) and a batch of two (a list of ids): one PNG and one .pt per
    sample, named after the label file; the PNG decodes to predict's labels with the given palette, the .pt is `final`."""
    from semivl_amd.evaluate import predict
    from semivl_amd.report import evaluate_report, voc_palette
    model, img, mask, cfg, _ = toy
    ids = ["JPEGImages/a.jpg SegmentationClass/sub/a.png", "JPEGImages/b.jpg SegmentationClass/b.png"]
    loaders = {"one": _loader(img, mask, ids), "two": [(img, mask, ids)]}
    pal = voc_palette(256) if palette is None else palette
    for tag, loader in loaders.items():
        with torch.no_grad():
            outs = [predict(model, i.to(dev), m.to(dev), "original", cfg, return_logits=True) for i, m, _ in loader]
        pred, final = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        pp, lp = str(tmp_path / tag / "pred"), str(tmp_path / tag / "logits" / "deep")
        rep = evaluate_report(model, loader, "original", cfg, pred_path=pp, logit_path=lp, palette=palette, workers=3)
        assert np.array_equal(rep.table.reshape(-1), R.confusion_ref(pred, mask.to(dev), cfg["nclass"]).cpu().numpy())
        assert sorted(os.listdir(pp)) == ["a.png", "b.png"] and sorted(os.listdir(lp)) == ["a.pt", "b.pt"]
        for i, name in enumerate("ab"):
            arr, got_pal = _read_png(os.path.join(pp, name + ".png"))
            assert arr.dtype == np.uint8 and np.array_equal(arr, pred[i].cpu().numpy().astype(np.uint8))
            assert got_pal[:len(pal)] == pal
            f = torch.load(os.path.join(lp, name + ".pt"))
            assert f.device.type == "cpu" and f.dtype == torch.float32 and f.shape == (1,) + tuple(final.shape[1:])
            assert torch.equal(f[0], final[i].cpu())
    # only one of the two
    only = str(tmp_path / "only")
    evaluate_report(model, loaders["one"], "original", cfg, logit_path=only)
    assert sorted(os.listdir(only)) == ["a.pt", "b.pt"]


def test_export_errors_surface(dev, toy, tmp_path):
    from semivl_amd.report import evaluate_report
    model, img, mask, cfg, _ = toy
    bad_ext = _loader(img, mask, ["a.jpg lbl/a.png", "b.jpg lbl/b.no_such_format"])
    with pytest.raises(ValueError, match="no_such_format|unknown file extension"):         # raised by PIL inside a writer thread
        evaluate_report(model, bad_ext, "original", cfg, pred_path=str(tmp_path / "p"))
    assert os.path.exists(tmp_path / "p" / "a.png")          # the other writers were joined, not abandoned
    with pytest.raises(ValueError, match="one id"):
        evaluate_report(model, _loader(img, mask), "original", cfg, pred_path=str(tmp_path / "q"))
    with pytest.raises(ValueError, match="one id"):
        evaluate_report(model, [(img, mask, ["a.jpg a.png"])], "original", cfg, logit_path=str(tmp_path / "q"))
    with pytest.raises(ValueError, match="nclass = 300 > 256"):
        evaluate_report(model, _loader(img, mask), "original", dict(cfg, nclass=300), pred_path=str(tmp_path / "r"))
    with pytest.raises(ValueError, match="palette"):
        evaluate_report(model, _loader(img, mask), "original", cfg, palette=[1, 2])
    with pytest.raises(ValueError, match="eval_report.*'metric'"):
        evaluate_report(model, _loader(img, mask), "original", dict(cfg, eval_report=dict(metric=[])))
    with pytest.raises(ValueError):
        evaluate_report(model, _loader(img, mask), "whole", cfg)


def _tiny_run(tmp_path):
    """A three-image VOC-style dataset, a yaml config of the tiny product VLM and a checkpoint of seeded weights."""
    import yaml
    from PIL import Image
    from golden_util import seeded_state
    from semivl_amd.checkpoint import save_checkpoint
    from semivl_amd.model.builder import build_model, builtin_model_cfg
    g = torch.Generator().manual_seed(5)
    root = tmp_path / "data"
    os.makedirs(root / "JPEGImages")
    os.makedirs(root / "SegmentationClass")
    ids = []
    for i, (h, w) in enumerate([(160, 150), (144, 170), (150, 136)]):
        img = torch.nn.functional.avg_pool2d(torch.randn(1, 3, h, w, generator=g), 9, stride=1, padding=4)[0]
        img = ((img / img.std()) * 60 + 128).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
        lbl = torch.randint(0, 21, (h // 8 + 1, w // 8 + 1), generator=g).repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w]
        lbl[:, :5] = 255
        Image.fromarray(img).save(root / "JPEGImages" / f"im{i}.png")
        Image.fromarray(lbl.to(torch.uint8).numpy()).save(root / "SegmentationClass" / f"im{i}.png")
        ids.append(f"JPEGImages/im{i}.png SegmentationClass/im{i}.png")
    (tmp_path / "val.txt").write_text("\n".join(ids) + "\n")
    m = copy.deepcopy(builtin_model_cfg("vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb"))["model"]
    m["backbone"].update(img_size=(128, 128), embed_dims=64, num_layers=3, num_heads=1, out_indices=[0, 1, 3])
    m["decode_head"].update(img_size=128, num_classes=21, text_channels=32, up_channels=(32, 16), skip_in_channels=(64, 64),
                            skip_channels=(16, 16), num_heads=1, channels=32)
    cfg = dict(dataset="pascal", data_root=str(root), val_id_path=str(tmp_path / "val.txt"), nclass=21, crop_size=128,
               model="mmseg.vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb", text_embedding_variant="single", mcc_text="concept4_single",
               pl_text="single", disable_dropout=True, fp_rate=0.5, allow_random_init=True, pretrained=None,
               model_args=dict(backbone=m["backbone"], decode_head=m["decode_head"], pretrained=None),
               eval_report=dict(metrics=["mIoU", "mFscore"]))
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.dump(cfg, f)
    model = build_model(dict(cfg, clip_encoder=None))
    sd = seeded_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 21, 150.0)
    model.load_state_dict(sd, strict=True)
    save_checkpoint(str(tmp_path / "ckpt.pth"), model, None, 3)
    return cfg, ids


def test_eval_tool_on_a_three_image_dataset(dev, tmp_path, capsys):
    from semivl_amd.checkpoint import load_checkpoint
    from semivl_amd.data import GpuAugmenter, ValLoader
    from semivl_amd.evaluate import evaluate, predict
    from semivl_amd.model.builder import build_model
    from semivl_amd.tools.eval import main
    cfg, ids = _tiny_run(tmp_path)
    rep = main(["--config", str(tmp_path / "cfg.yaml"), "--save-path", str(tmp_path / "ckpt.pth"),
                "--pred-path", str(tmp_path / "pred"), "--report-json", str(tmp_path / "out" / "report.json")])
    out = capsys.readouterr().out
    cfg = dict(cfg, clip_encoder=None)
    model = build_model(cfg).to(dev)
    assert load_checkpoint(str(tmp_path / "ckpt.pth"), model) == 3
    loader = ValLoader(cfg, GpuAugmenter.from_cfg(cfg, device=dev))
    assert len(loader) == 3 and [i for _, _, i in loader] == ids
    assert [len(ValLoader(cfg, GpuAugmenter.from_cfg(cfg, device=dev), r, 2)) for r in (0, 1)] == [2, 1]      # no padding
    assert ValLoader(cfg, GpuAugmenter.from_cfg(cfg, device=dev), 1, 2).ids == ids[1::2]
    m, iou = evaluate(model, loader, "original", cfg)
    assert rep.miou == m and np.array_equal(rep.iou_class, iou) and 0.0 < m < 100.0
    assert "***** Evaluation original ***** >>>> MeanIoU: {:.2f}".format(m) in out
    assert "Load from checkpoint at epoch 3" in out and rep.format_table() in out
    d = json.load(open(tmp_path / "out" / "report.json"))
    assert d["miou"] == m and d["eval_mode"] == "original" and d["images"] == 3 and d["nclass"] == 21
    assert d["table"] == rep.table.tolist() and d["spec"]["metrics"] == ["mIoU", "mFscore"]
    assert sorted(os.listdir(tmp_path / "pred")) == ["im0.png", "im1.png", "im2.png"]
    with torch.no_grad():
        for k, (img, mask, id_) in enumerate(loader):
            assert img.shape[:2] == (1, 3) and mask.shape[0] == 1 and mask.dtype == torch.int64 and img.is_cuda
            arr, _ = _read_png(tmp_path / "pred" / f"im{k}.png")
            assert np.array_equal(arr, predict(model, img, mask, "original", cfg)[0].cpu().numpy().astype(np.uint8))
    # --eval-mode and 'none'
    rep2 = main(["--config", str(tmp_path / "cfg.yaml"), "--save-path", "none", "--eval-mode", "sliding_window"])
    out = capsys.readouterr().out
    assert "NO CHECKPOINT SPECIFIED" in out and "***** Evaluation sliding_window *****" in out and rep2.K == 21
