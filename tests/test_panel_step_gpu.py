"""semivl_train_step(..., panel=StepPanel(...)) on the tiny VLG model of the other step tests, exact fp32 GEMMs (mode 0) and
the split emulation (mode 6), guided and with maskclip_consistency_lambda = 0: the canvas equals the restatement
(tests/panel_ref.py) built from the batch, `aux`, train.cutmix_mask of aux's maps and the step's own _smax of the logits,
byte for byte; the PNG on disk decodes to the canvas; and the step computes bit for bit what it computes without a panel."""
import os

import numpy as np
import pytest
import torch

import panel_ref as P
from test_ema_step_gpu import ADAMW, AUX_KEYS, CFG, _batch, _bits, _tiny

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 6])
def mode(request):
    from semivl_amd import ops
    ops.set_gemm_emulation(request.param)
    yield request.param
    ops.set_gemm_emulation(0)


def _step(dev, guided, out_dir, monkeypatch):
    """One step on fresh weights; every call of the step's own _smax is recorded as (logits, up, label map)."""
    from semivl_amd import train
    from semivl_amd.optim import optimizer_from_cfg
    from semivl_amd.panel import StepPanel
    hip, z, c = _tiny(dev)
    opt = optimizer_from_cfg(hip, dict(optimizer=ADAMW))
    cfg = CFG if guided else dict(CFG, maskclip_consistency_lambda=0)
    batch, masks = _batch(dev, z, c)
    panel = StepPanel(out_dir, rank=0) if out_dir is not None else None
    calls, real = [], train._smax

    def spy(pred, up):
        out = real(pred, up)
        calls.append((pred, up, out[1]))
        return out
    monkeypatch.setattr(train, "_smax", spy)
    try:
        losses, aux = train.semivl_train_step(hip, batch, 7, 50, cfg, optimizer=opt, fp_masks=masks, return_aux=True,
                                              panel=panel)
    finally:
        monkeypatch.setattr(train, "_smax", real)
    torch.cuda.synchronize()
    return hip, losses.clone(), aux, batch, opt.p.clone(), panel, calls


@pytest.mark.parametrize("guided", [True, False])
def test_canvas_is_what_the_step_trains_on(dev, mode, guided, tmp_path, monkeypatch):
    from PIL import Image
    from semivl_amd.report import voc_palette
    from semivl_amd.train import _smax, cutmix_mask
    _, l0, aux0, _, p0, _, calls0 = _step(dev, guided, None, monkeypatch)
    hip, l1, aux, batch, p1, panel, calls = _step(dev, guided, str(tmp_path / "debug"), monkeypatch)
    # 1. no interference: losses, both logit gradients, the updated parameters; aux gets no new key; two more _smax launches
    assert _bits(l1, l0) and _bits(aux["dl4"], aux0["dl4"]) and _bits(aux["dls"], aux0["dls"]) and _bits(p1, p0)
    assert set(aux) == set(aux0) == AUX_KEYS and len(calls) == len(calls0) + 2
    # 2. the canvas: the restatement on the batch (img_s1 / img_s2 were cut in place), aux's maps, cutmix_mask of them and
    # _smax of the logits the step held -- [x, w_fp] of the first decode and [s1, s2] of the second, at the step's `up`
    B, _, H, W = batch["img_x"].shape
    canvas = panel.canvas
    assert canvas.dtype == torch.uint8 and tuple(canvas.shape) == (B, (4 if guided else 3) * H, 4 * W, 3)
    (p4, up4, _), (ps, ups, _) = calls[-2:]
    assert aux["upsample_in_loss"] and up4 == ups == (H, W, bool(hip.align_corners)), "the tiny model's logits stay at head resolution"
    assert p4.shape[0] == 2 * B and ps.shape[0] == 2 * B and tuple(p4.shape[2:]) == tuple(aux["dl4"].shape[2:]) != (H, W)
    cpu = lambda t: t.cpu().numpy()
    pm4, pms = cpu(_smax(p4, up4)[1]), cpu(_smax(ps, ups)[1])
    mix = lambda a, b, k: cpu(cutmix_mask(a, b, batch[k]))
    rows = [[pm4[:B], pms[:B], pms[B:], pm4[B:]],
            [cpu(batch["mask_x"]), mix(aux["mask_w"], aux["mask_w_other"], "mix1"), mix(aux["mask_w"], aux["mask_w_other"], "mix2"),
             cpu(aux["mask_w"])]]
    if guided:
        rows.append([None, mix(aux["mclip"], aux["mclip_other"], "mix1"), mix(aux["mclip"], aux["mclip_other"], "mix2"),
                     cpu(aux["mclip"])])
    else:
        assert aux["mclip"] is None
    pal = np.array(voc_palette(256), np.uint8).reshape(-1, 3)
    want = P.canvas([cpu(batch[k]) for k in ("img_x", "img_s1", "img_s2", "img_w")], rows, pal)
    got = cpu(canvas)
    assert np.array_equal(got, want)
    if guided:
        assert (got[:, 3 * H:, :W] == 255).all()
    # the FP tile of the label row is mask_w itself: the map this kernel made from pred_w and the step trained on
    assert np.array_equal(got[:, 2 * H:3 * H, 3 * W:], P.label_tile(cpu(aux["mask_w"]), pal))
    # 3. the files decode to the canvas
    panel.close()
    files = sorted(os.listdir(tmp_path / "debug"))
    assert files == [f"0000007_0-{b}.png" for b in range(B)] and [os.path.basename(f) for f in panel.files] == files
    for b, name in enumerate(files):
        with Image.open(tmp_path / "debug" / name) as im:
            assert im.mode == "RGB" and np.array_equal(np.array(im), got[b])


def test_prediction_tiles_are_the_steps_own_smax(dev, tmp_path):
    """The panel's capture with the logits in hand: every prediction tile is _smax(pred, up)'s label map, exactly."""
    from semivl_amd import ops
    from semivl_amd.panel import StepPanel
    from semivl_amd.report import voc_palette
    from semivl_amd.train import _panel_capture, _smax
    from types import SimpleNamespace
    ops.set_gemm_emulation(0)
    B, N, h, w, H, W = 2, 21, 32, 32, 128, 128          # (the tiny model's geometry: the fused-resize kernels take it)
    g = torch.Generator().manual_seed(3)
    preds4 = torch.randn(3 * B, N, h, w, generator=g).to(dev)
    preds_s = torch.randn(2 * B, N, h, w, generator=g).to(dev)
    maps = lambda: torch.randint(0, N, (B, H, W), generator=g).to(dev)
    b = {k: torch.randn(B, 3, H, W, generator=g).to(dev) for k in ("img_x", "img_s1", "img_s2", "img_w")}
    b["mask_x"] = maps()
    lab = SimpleNamespace(mask_w=maps(), mclip=maps())
    mix = SimpleNamespace(mw=(maps(), maps()), mc=(maps(), maps()))
    pal = np.array(voc_palette(256), np.uint8).reshape(-1, 3)
    cpu = lambda t: t.cpu().numpy()
    for up in ((H, W, False), (H, W, True), None):
        if up is None:
            preds4, preds_s = (torch.randn(n * B, N, H, W, generator=g).to(dev) for n in (3, 2))
        for guided in (True, False):
            panel = StepPanel(str(tmp_path / f"{up}-{guided}"))
            _panel_capture(panel, 3, b, preds4, preds_s, lab, mix, SimpleNamespace(B=B, up=up, guided=guided))
            pm = [_smax(p.contiguous(), up)[1] for p in (preds4[B:2 * B], preds_s[:B], preds_s[B:], preds4[2 * B:])]
            rows = [[cpu(m) for m in pm], [cpu(m) for m in (b["mask_x"], mix.mw[0], mix.mw[1], lab.mask_w)]]
            if guided:
                rows.append([None] + [cpu(m) for m in (mix.mc[0], mix.mc[1], lab.mclip)])
            want = P.canvas([cpu(b[k]) for k in ("img_x", "img_s1", "img_s2", "img_w")], rows, pal)
            assert np.array_equal(cpu(panel.canvas), want)
            panel.close()


def test_panel_none_and_errors(dev, tmp_path):
    import inspect
    from semivl_amd.panel import StepPanel, canvas_shape, palette_from_cfg
    from semivl_amd.report import voc_palette
    from semivl_amd.train import semivl_train_step
    assert inspect.signature(semivl_train_step).parameters["panel"].default is None
    assert canvas_shape(2, 8, 6, True) == (2, 32, 24, 3) and canvas_shape(2, 8, 6, False) == (2, 24, 24, 3)
    assert palette_from_cfg({}) == voc_palette(256) and palette_from_cfg(dict(palette=[1, 2, 3])) == [1, 2, 3]
    for bad in ([1, 2], "abc", [1, 2, 300], [True, 0, 0], []):
        with pytest.raises(ValueError, match="palette"):
            palette_from_cfg(dict(palette=bad))
    with pytest.raises(ValueError, match="palette"):
        StepPanel(str(tmp_path / "x"), palette=[1, 2])
    # a writer's error surfaces in close(), not in the step thread; the other files are written
    panel = StepPanel(str(tmp_path / "ok"))
    img = [torch.zeros(1, 3, 4, 4, device=dev)] * 4
    rows = [[torch.zeros(1, 4, 4, dtype=torch.int64, device=dev)] * 4] * 2
    os.makedirs(tmp_path / "ok" / "0000002_0-0.png")                     # a directory where the second file goes
    panel.capture(1, img, rows)
    panel.capture(2, img, rows)
    panel.capture(3, img, rows)
    with pytest.raises(OSError):
        panel.close()
    assert os.path.isfile(tmp_path / "ok" / "0000001_0-0.png") and os.path.isfile(tmp_path / "ok" / "0000003_0-0.png")
    with pytest.raises(ValueError, match="4 images"):
        StepPanel(str(tmp_path / "y")).render(img[:3], rows)
