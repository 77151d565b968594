"""CPU: the float64 restatement of the labelled cross entropy with label smoothing and class weights (tests/celoss_ref.py)
against torch's own F.cross_entropy(weight=, ignore_index=255, label_smoothing=) and its float64 autograd; the reading of
cfg['criterion'] (semivl_amd.train.celoss_kwargs); and torch's own fp32 loss inside the limits the GPU tests hold the
kernels to, on those tests' inputs (the limits are not tighter than fp32 arithmetic itself)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import celoss_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _weights(kind, N):
    g = torch.Generator().manual_seed(3 + N)
    if kind == "none":
        return None
    w = torch.rand(N, generator=g, dtype=torch.float64) + 0.5
    if kind == "zero":
        w[N - 1] = 0.0
    return w


@pytest.mark.parametrize("N", [2, 21])
@pytest.mark.parametrize("kind", ["none", "random", "zero"])
@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
def test_restatement_equals_torch_float64(eps, kind, N):
    w = _weights(kind, N)
    x, t = R.logits_and_target((2, N, 12, 9), (2, 12, 9), N, seed=5)
    xd = x.double().requires_grad_(True)
    ref = F.cross_entropy(xd, t, weight=w, ignore_index=255, label_smoothing=eps)
    (gref,) = torch.autograd.grad(ref, xd)
    got = R.celoss(x, t, eps, w)
    assert abs(got["loss"].item() - ref.item()) < 1e-12
    assert (got["grad"] - gref).abs().max().item() < 1e-12
    assert abs(got["num"].sum().item() / got["D"].item() - ref.item()) < 1e-12
    wt = torch.ones(N, dtype=torch.float64) if w is None else w
    assert abs(got["D"].item() - wt[t[t != 255]].sum().item()) < 1e-12
    assert (got["num"][t == 255] == 0).all() and (got["grad"].movedim(1, -1)[t == 255] == 0).all()
    # factor 0.5: the labelled branch of the semi-supervised step (semivl.py:319)
    assert (R.celoss(x, t, eps, w, factor=0.5)["grad"] - 0.5 * gref).abs().max().item() < 1e-12
    # the resized form, both corner conventions: loss, and the gradient at the head's resolution
    for align in (False, True):
        xl = x[:, :, :5, :4].contiguous().double().requires_grad_(True)
        up = F.interpolate(xl, size=(12, 9), mode="bilinear", align_corners=align)
        assert (R.resize(xl, 12, 9, align) - up).abs().max().item() < 1e-12
        ref = F.cross_entropy(up, t, weight=w, ignore_index=255, label_smoothing=eps)
        (gref,) = torch.autograd.grad(ref, xl)
        got = R.celoss_up(xl, 12, 9, align, t, eps, w)
        assert abs(got["loss"].item() - ref.item()) < 1e-12
        assert (got["grad"] - gref).abs().max().item() < 1e-12


def test_every_target_ignored_gives_zero_gradient():
    x, t = R.logits_and_target((1, 4, 30), (1, 30), 4, seed=1)
    t[:] = 255
    got = R.celoss(x, t, 0.1, None)
    assert torch.isnan(got["loss"]) and (got["grad"] == 0).all() and got["D"].item() == 0


# ------------------------------------------------------------------------------------------------ cfg['criterion']
def test_celoss_kwargs_on_the_generated_dicts():
    from semivl_amd.train import celoss_kwargs
    rows = json.load(open(os.path.join(HERE, "golden", "experiment_cfgs.json")))["experiments"]
    assert len(rows) >= 4
    for cfg in rows.values():
        assert cfg["criterion"]["name"] == "CELoss"
        assert celoss_kwargs(cfg, cfg["nclass"]) == (0.0, None)
    assert celoss_kwargs({}, 21) == (0.0, None)
    assert celoss_kwargs(dict(criterion=dict(name="CELoss")), 21) == (0.0, None)
    # OHEM's kwargs go to ProbOhemCrossEntropy2d, which has no such arguments; other names stay the plain loss
    assert celoss_kwargs(dict(criterion=dict(name="OHEM", kwargs=dict(ignore_index=255, thresh=0.7, min_kept=100))), 21) == (0.0, None)
    assert celoss_kwargs(dict(criterion=dict(name="Other", kwargs=dict(label_smoothing=0.3))), 21) == (0.0, None)


@pytest.mark.parametrize("make", [list, tuple, np.asarray, torch.tensor, lambda v: np.asarray(v, dtype=np.float32)])
def test_celoss_kwargs_reads_valid_settings(make):
    from semivl_amd.train import celoss_kwargs
    vals = [0.5, 1.0, 1.5, 0.0, 2.0]
    eps, w = celoss_kwargs(dict(criterion=dict(name="CELoss", kwargs=dict(ignore_index=255, label_smoothing=0.1,
                                                                           weight=make(vals)))), 5)
    assert eps == 0.1 and isinstance(eps, float)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.tolist() == vals
    for e in (0, 1, 0.0, 1.0, np.float32(0.25)):
        assert celoss_kwargs(dict(criterion=dict(name="CELoss", kwargs=dict(label_smoothing=e))), 5) == (float(e), None)
    # every other key is not read (as before)
    assert celoss_kwargs(dict(criterion=dict(name="CELoss", kwargs=dict(ignore_index=7, reduction="sum"))), 5) == (0.0, None)


@pytest.mark.parametrize("eps", [-0.1, 1.5, "0.1", None, True, float("nan")])
def test_celoss_kwargs_refuses_bad_label_smoothing(eps):
    from semivl_amd.train import celoss_kwargs
    with pytest.raises(ValueError, match="label_smoothing"):
        celoss_kwargs(dict(criterion=dict(name="CELoss", kwargs=dict(label_smoothing=eps))), 21)


def test_celoss_kwargs_refuses_a_weight_of_the_wrong_length():
    from semivl_amd.train import celoss_kwargs
    with pytest.raises(ValueError, match=r"19.*21"):
        celoss_kwargs(dict(criterion=dict(name="CELoss", kwargs=dict(weight=[1.0] * 19))), 21)
    with pytest.raises(ValueError, match=r"42.*21"):
        celoss_kwargs(dict(criterion=dict(name="CELoss", kwargs=dict(weight=np.ones((2, 21))))), 21)


def test_steps_refuse_bad_kwargs_before_touching_anything():
    """Both steps read the kwargs first: a bad value raises before the batch or the model is used."""
    from semivl_amd.train import semivl_train_step, supervised_train_step

    class M:
        num_classes = 21
    bad = dict(criterion=dict(name="CELoss", kwargs=dict(label_smoothing=1.5)))
    with pytest.raises(ValueError, match="label_smoothing"):
        supervised_train_step(M(), dict(img_x=torch.zeros(1, 3, 8, 8), mask_x=torch.zeros(1, 8, 8, dtype=torch.int64)), 1, 10, bad)
    with pytest.raises(ValueError, match="label_smoothing"):
        semivl_train_step(M(), dict(img_x=torch.zeros(1, 3, 8, 8)), 1, 10, bad)


# ------------------------------------------------------------------------------------------------ the GPU limits
def _check_fp32(ref, loss32, grad32, g):
    assert abs(loss32 - ref["loss"].item()) < R.LOSS_TOL
    err = (grad32.double() - ref["grad"]).abs()
    lim = R.GRAD_ATOL_G * g + R.GRAD_RTOL * ref["grad"].abs()
    return (err / lim).max().item()


@pytest.mark.parametrize("name", R.SETTINGS)
def test_torch_fp32_lies_inside_the_gpu_limits(name):
    """F.cross_entropy in fp32 (and fp32 F.interpolate in front of it) against the float64 restatement, on the inputs of
    tests/test_celoss_kernels_gpu.py: inside the limits the kernels are held to."""
    worst = 0.0
    for (B, N, HW) in R.FUSED_SHAPES:
        eps, w = R.setting(name, N)
        x, t = R.logits_and_target((B, N, HW), (B, HW), N, seed=11)
        ref = R.celoss(x, t, eps, w)
        x32 = x.clone().requires_grad_(True)
        l32 = F.cross_entropy(x32, t, weight=w, ignore_index=255, label_smoothing=eps)
        (g32,) = torch.autograd.grad(l32, x32)
        worst = max(worst, _check_fp32(ref, l32.item(), g32, 1.0 / ref["D"].item()))
    for (N, h, w_, H, W) in R.UP_GEOMS:
        for align in (False, True):
            eps, w = R.setting(name, N)
            x, t = R.logits_and_target((2, N, h, w_), (2, H, W), N, seed=12)
            ref = R.celoss_up(x, H, W, align, t, eps, w)
            x32 = x.clone().requires_grad_(True)
            up = F.interpolate(x32, size=(H, W), mode="bilinear", align_corners=align)
            l32 = F.cross_entropy(up, t, weight=w, ignore_index=255, label_smoothing=eps)
            (g32,) = torch.autograd.grad(l32, x32)
            worst = max(worst, _check_fp32(ref, l32.item(), g32, 1.0 / ref["D"].item()))
    print(f"\n[celoss limits] torch fp32 / limit, worst over shapes and geometries, {name}: {worst:.3f}")
    assert worst < 1.0
