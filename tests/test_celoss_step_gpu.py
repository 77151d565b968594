"""GPU: cfg['criterion'] = dict(name='CELoss', kwargs=dict(label_smoothing=, weight=)) in the two training steps, on the tiny
VLG model (the resize is fused into the loss) and the tiny DeepLabV3+ `ftap` model (resized logits, train-mode BatchNorm) of
tests/test_noguidance_gpu.py, exact fp32 GEMMs (mode 0) and the bf16 x 6 emulation (mode 6).

The step's own `pred_x` is the input of the float64 restatement (tests/celoss_ref.py): its loss must equal the step's loss_x
within 1e-5, and its gradient -- carried to the head's resolution through the resize's transpose where the step fuses the
resize -- must equal the gradient the step hands to autograd within the kernel limits of tests/test_celoss_kernels_gpu.py
(atol 4e-5 g, rtol 2e-4; g = factor / D with factor 1 in supervised_train_step and 0.5 in semivl_train_step).  Everything the
labelled launch does not write is bit-equal to the same step without the kwargs."""
import numpy as np
import pytest
import torch

import celoss_ref as R
from test_noguidance_gpu import dlv3p_case, grads_of, vlg_case, vlg_cfg, zero_grads

pytestmark = pytest.mark.gpu
SETTINGS = ["eps", "weights", "both"]


def kwargs_of(setting, N):
    w = R.setting("weights", N)[1]
    kw = dict(ignore_index=255)
    if setting in ("eps", "both"):
        kw["label_smoothing"] = 0.1
    if setting in ("weights", "both"):
        kw["weight"] = w.tolist()
    return kw, kw.get("label_smoothing", 0.0), (w if "weight" in kw else None)


def case(which, dev, tmp_path, monkeypatch):
    """model, cfg, batch, fp_masks and a copy of the state (BatchNorm buffers included: every run starts from it)"""
    if which == "vlg":
        model, _, batch, masks = vlg_case(dev)
        cfg = vlg_cfg()
    else:
        model, cfg, batch, masks = dlv3p_case(tmp_path, monkeypatch, dev)
        cfg = dict(cfg, maskclip_consistency_lambda=0)
    return model, cfg, batch, masks, {k: v.clone() for k, v in model.state_dict().items()}


def check_labelled(pred_x, mask_x, eps, w, factor, loss_x, dl_x, align, what):
    """loss and gradient of the labelled branch against the float64 restatement on the step's own pred_x"""
    ref = R.celoss(pred_x, mask_x, eps, w, factor=factor)
    g = factor / ref["D"].item()
    grad = ref["grad"]
    if tuple(dl_x.shape) != tuple(grad.shape):          # the step fused the resize: the gradient lives at the head's resolution
        grad = R.resize_transpose(grad, dl_x.shape[2], dl_x.shape[3], align)
    e_loss = abs(loss_x - ref["loss"].item())
    err = (dl_x.double().cpu() - grad).abs()
    ratio = (err / (R.GRAD_ATOL_G * g + R.GRAD_RTOL * grad.abs())).max().item()
    print(f"\n[{what}] loss_x {loss_x:.7f} (float64 of pred_x {ref['loss'].item():.7f}, |d| {e_loss:.2e} / {R.LOSS_TOL:.0e}); "
          f"gradient error / limit {ratio:.4f}")
    assert e_loss < R.LOSS_TOL
    assert torch.allclose(dl_x.double().cpu(), grad, atol=R.GRAD_ATOL_G * g, rtol=R.GRAD_RTOL), ratio


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("mode", [0, 6])
@pytest.mark.parametrize("which", ["vlg", "dlv3p"])
def test_supervised_step_with_celoss_kwargs(dev, tmp_path, monkeypatch, which, mode, setting):
    from semivl_amd import ops
    from semivl_amd.train import FusedAdamW, supervised_train_step
    ops.set_gemm_emulation(mode)
    try:
        model, cfg, batch, _, state = case(which, dev, tmp_path, monkeypatch)
        kw, eps, w = kwargs_of(setting, model.num_classes)
        cfg = dict(cfg, criterion=dict(name="CELoss", kwargs=kw))
        sup = dict(img_x=batch["img_x"], mask_x=batch["mask_x"])
        loss, aux = supervised_train_step(model, sup, 1, 10, cfg, return_aux=True)
        torch.cuda.synchronize()
        assert aux["upsample_in_loss"] == (which == "vlg") and aux["mask_x_ohem"] is None
        check_labelled(aux["pred_x"], batch["mask_x"], eps, w, 1.0, loss.item(), aux["dlogits"], model.align_corners,
                       f"supervised {which} mode {mode} {setting}")
        g = grads_of(model)
        assert g and all(bool(torch.isfinite(v).all()) for v in g.values())
        # the kwargs change the step: not the plain loss
        model.load_state_dict(state)
        zero_grads(model)
        plain = supervised_train_step(model, sup, 1, 10, dict(cfg, criterion=dict(name="CELoss", kwargs=dict(ignore_index=255))))
        assert abs(plain.item() - loss.item()) > 1e-4
        # two runs, bit-equal; then one optimizer step moves the parameters
        model.load_state_dict(state)
        zero_grads(model)
        loss2 = supervised_train_step(model, sup, 1, 10, cfg)
        assert torch.equal(loss2, loss)
        for k, v in grads_of(model).items():
            assert torch.equal(v, g[k]), k
        model.load_state_dict(state)
        zero_grads(model)
        opt = FusedAdamW(model, dict(type="AdamW", lr=1e-2, weight_decay=0.01))
        before = {k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
        loss3 = supervised_train_step(model, sup, 1, 10, cfg, optimizer=opt)
        torch.cuda.synchronize()
        assert torch.equal(loss3, loss)
        moved = [k for k, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[k])]
        assert len(moved) == len(before), sorted(set(before) - set(moved))[:5]
    finally:
        ops.set_gemm_emulation(0)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("mode", [0, 6])
@pytest.mark.parametrize("which", ["vlg", "dlv3p"])
def test_semivl_step_with_celoss_kwargs(dev, tmp_path, monkeypatch, which, mode, setting):
    from semivl_amd import ops
    from semivl_amd.train import FusedAdamW, semivl_train_step
    ops.set_gemm_emulation(mode)
    try:
        model, cfg, batch, masks, state = case(which, dev, tmp_path, monkeypatch)
        B = batch["img_x"].shape[0]
        kw, eps, w = kwargs_of(setting, model.num_classes)
        cfg_kw = dict(cfg, criterion=dict(name="CELoss", kwargs=kw))

        def run(c, **more):
            model.load_state_dict(state)
            zero_grads(model)
            out = semivl_train_step(model, {k: v.clone() for k, v in batch.items()}, 1, 10, c, fp_masks=masks, **more)
            torch.cuda.synchronize()
            return out

        losses0, aux0 = run(cfg, return_aux=True)
        losses, aux = run(cfg_kw, return_aux=True)
        assert aux["upsample_in_loss"] == aux0["upsample_in_loss"] == (which == "vlg")
        # the labelled branch: loss_x and the gradient of pred_x, factor 0.5 (semivl.py:319)
        check_labelled(aux["pred_x"], batch["mask_x"], eps, w, 0.5, losses[1].item(), aux["dl4"][B:2 * B], model.align_corners,
                       f"semivl {which} mode {mode} {setting}")
        assert abs(losses[1].item() - losses0[1].item()) > 1e-4
        # losses[0] from its parts, in the fp32 order of svl_semivl_loss (no guidance: lambda = 0)
        lv = losses.cpu().numpy().astype(np.float32)
        half, quarter = np.float32(0.5), np.float32(0.25)
        want = (lv[1] + lv[2] * quarter + lv[3] * quarter + lv[4] * half) / np.float32(2.0)
        assert abs(lv[0] - want) <= 2.0 ** -22 * abs(want), (lv[0], want)
        # only the labelled launch changed: every other output is bit-equal to the step without the kwargs
        assert torch.equal(losses[2:], losses0[2:])
        assert torch.equal(aux["dls"], aux0["dls"])
        assert torch.equal(aux["dl4"][:B], aux0["dl4"][:B]) and torch.equal(aux["dl4"][2 * B:], aux0["dl4"][2 * B:])
        for k in ("pred_x", "pred_s1", "pred_w", "pred_w_other", "mask_w", "mask_w_other", "conf_w"):
            assert torch.equal(aux[k], aux0[k]), k
        assert not torch.equal(aux["dl4"][B:2 * B], aux0["dl4"][B:2 * B])
        # one optimizer step moves the parameters
        model.load_state_dict(state)
        zero_grads(model)
        opt = FusedAdamW(model, dict(type="AdamW", lr=1e-2, weight_decay=0.01))
        before = {k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
        losses3 = semivl_train_step(model, {k: v.clone() for k, v in batch.items()}, 1, 10, cfg_kw, optimizer=opt, fp_masks=masks)
        torch.cuda.synchronize()
        assert torch.equal(losses3, losses)
        moved = [k for k, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[k])]
        assert len(moved) == len(before), sorted(set(before) - set(moved))[:5]
    finally:
        ops.set_gemm_emulation(0)


@pytest.mark.parametrize("mode", [0, 6])
@pytest.mark.parametrize("which", ["vlg", "dlv3p"])
def test_zero_smoothing_and_no_weight_change_nothing(dev, tmp_path, monkeypatch, which, mode):
    """label_smoothing=0.0 without a weight: both steps return bit for bit what they return without the keys."""
    from semivl_amd import ops
    from semivl_amd.train import semivl_train_step, supervised_train_step
    ops.set_gemm_emulation(mode)
    try:
        model, cfg, batch, masks, state = case(which, dev, tmp_path, monkeypatch)
        sup = dict(img_x=batch["img_x"], mask_x=batch["mask_x"])
        outs = []
        for c in (cfg, dict(cfg, criterion=dict(name="CELoss", kwargs=dict(ignore_index=255, label_smoothing=0.0)))):
            model.load_state_dict(state)
            zero_grads(model)
            l_sup = supervised_train_step(model, sup, 1, 10, c).clone()
            g_sup = grads_of(model)
            model.load_state_dict(state)
            zero_grads(model)
            l_semi = semivl_train_step(model, {k: v.clone() for k, v in batch.items()}, 1, 10, c, fp_masks=masks).clone()
            torch.cuda.synchronize()
            outs.append((l_sup, g_sup, l_semi, grads_of(model)))
        (a_sup, ga_sup, a_semi, ga_semi), (b_sup, gb_sup, b_semi, gb_semi) = outs
        assert torch.equal(a_sup, b_sup) and torch.equal(a_semi, b_semi)
        for ga, gb in ((ga_sup, gb_sup), (ga_semi, gb_semi)):
            assert ga.keys() == gb.keys() and len(ga) > 5
            for k in ga:
                assert torch.equal(ga[k], gb[k]), k
    finally:
        ops.set_gemm_emulation(0)
