"""GPU: training without MaskCLIP guidance (`maskclip_consistency_lambda=0`, `clip_encoder=None`: experiment 41's rows) and
the labelled-only baseline `supervised_train_step`, against tests/golden/semivl_noguidance.npz -- the FLOAT64 run of the
reference's own modules (tests/golden/gen_golden_noguidance.py; cases A / C: the VLG row at the 'tiny' dimensions, B / D:
the DeepLabV3+ `ftap` row at crop 64, 5 classes, B = 2 with train-mode BatchNorm).

Limits: the ones the model tests of this repository use (tests/test_model_gpu.py, tests/test_ohem_gpu.py) -- losses 1e-3,
gradient norms 2e-3, full gradients 5e-3 relative max, BatchNorm running statistics 1e-3; label maps bit-exact outside the
fixture's tie masks.  The reference's own float32 run lies 8e-7 (losses), 6e-6 (gradient norms), 4e-5 (full gradients) and
5e-7 (running statistics) from its float64 run.  Measured values are printed (-s)."""
import ast
import functools
import json
import os

import numpy as np
import pytest
import torch

import noguidance_ref as R
from golden_util import (HERE, MCC_TEXT, TEXT, assert_labels, build_hip, fixture_batch, fixture_fp_masks, fixture_state,
                         seeded_state, smooth_batch)

pytestmark = pytest.mark.gpu
VLG, FT, FTAP = ("mmseg.vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb", "mmseg.vlm-dlv3p-bn12-sk4-ft-mcvitb",
                 "mmseg.vlm-dlv3p-bn12-sk4-ftap-mcvitb")
LOSS_TOL, NORM_TOL, GRAD_TOL, STAT_TOL = 1e-3, 2e-3, 5e-3, 1e-3


def to_dev(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


@functools.lru_cache(None)
def golden():
    z = np.load(os.path.join(HERE, "golden", "semivl_noguidance.npz"), allow_pickle=False)
    return z, ast.literal_eval(str(z["cfg"])), ast.literal_eval(str(z["dlv3p/cfg"]))


def null_row(model):
    rows = json.load(open(os.path.join(HERE, "golden", "experiment41_cfgs.json")))
    return next(c for c in rows.values() if c["model"] == model and c["clip_encoder"] is None)


def tiny_row_model(tmp_path, monkeypatch, dev, model, crop=64, nclass=5, **over):
    """A row of experiment 41 AS WRITTEN (its own clip_encoder / maskclip_consistency_lambda / mcc_loss_reduce) at crop 64
    with 5 classes: build_model resolves the text embeddings relative to the working directory first, so a 5-class
    embedding file there stands in for the 21-class one of the package (tests/test_dlv3p_gpu.py::_tiny_model)."""
    from semivl_amd.model.builder import build_model
    d = tmp_path / "configs" / "_base_" / "datasets" / "text_embedding"
    d.mkdir(parents=True, exist_ok=True)
    t = torch.randn(nclass, 512, generator=torch.Generator().manual_seed(5))
    np.save(d / "voc12_wbg_single.npy", (t / t.norm(dim=1, keepdim=True)).numpy().astype(np.float16))
    monkeypatch.chdir(tmp_path)
    cfg = dict(null_row(model), crop_size=crop, nclass=nclass, allow_random_init=True, **over)
    torch.manual_seed(11)
    return build_model(cfg).to(dev), cfg


def row_fp_masks(model, B, dev):
    chans = (768, 768, 512) if model == VLG else (768, 512)      # F.dropout2d's call order (builder.py:80-85)
    return [(torch.rand(2 * B, c, generator=torch.Generator().manual_seed(7 + i)) < 0.5).float().to(dev)
            for i, c in enumerate(chans)]


def build_hip_unguided(c):
    """golden_util.build_hip without the guidance encoder (cfg['clip_encoder'] = None)."""
    import copy
    from semivl_amd.model.builder import VLM, builtin_model_cfg
    mcfg = copy.deepcopy(builtin_model_cfg(VLG[6:]))["model"]
    S = c["S"]
    mcfg["backbone"].update(img_size=(S, S), embed_dims=c["embed"], num_layers=c["layers"], num_heads=c["heads"],
                            out_indices=c["out_indices"])
    mcfg["backbone"].pop("pretrained", None)
    mcfg["decode_head"].update(img_size=S, num_classes=21, text_channels=c["text_channels"], up_channels=c["up"],
                               skip_in_channels=(c["embed"], c["embed"]), skip_channels=c["skip"],
                               num_heads=c["dec_heads"], channels=c["channels"])
    mcfg.pop("type")
    mcfg.pop("pretrained", None)
    return VLM(load_text_embedding=TEXT, load_mcc_text_embedding=MCC_TEXT, load_pl_text_embedding=TEXT, clip_encoder=None,
               maskclip_class_filter=None, **mcfg)


def vlg_case(dev):
    z, c, _ = golden()
    hip = build_hip_unguided(c)
    assert hip.clip_encoder is None
    sd = fixture_state(z, c, hip)                     # (asserts the weight checksum)
    assert list(sd) == [str(k) for k in z["state_keys"]]
    hip.load_state_dict(sd, strict=True)
    return hip.to(dev), sd, to_dev(fixture_batch(z, c), dev), [m.to(dev) for m in fixture_fp_masks(z, c)]


def vlg_cfg(**kw):
    _, c, _ = golden()
    return dict(dict(conf_thresh=c["conf_thresh"], conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean",
                     maskclip_consistency_lambda=0), **kw)


def dlv3p_case(tmp_path, monkeypatch, dev):
    """The model, cfg, inputs and channel masks of cases B / D: weights seeded in the fixture's key order (once per session)
    and inputs regenerated from the seeds, both checked against the fixture's checksums."""
    from oracle import semivl_oracle as O
    z, _, d = golden()
    keys = [str(k) for k in z["dlv3p/state_keys"]]
    model, cfg = tiny_row_model(tmp_path, monkeypatch, dev, FTAP, d["crop"], d["nclass"])
    own = model.state_dict()
    assert sorted(own) == sorted(keys)
    sd = _dlv3p_state(tuple((k, tuple(own[k].shape)) for k in keys), d["seed"])
    model.load_state_dict(sd, strict=True)
    batch = smooth_batch(O.synthetic_batch(d["B"], d["crop"], d["nclass"], seed=1234 + d["seed"]))
    assert abs(sum(v.double().sum().item() for v in batch.values()) - float(z["dlv3p/in_checksum"][0])) < 1e-6
    flat = torch.from_numpy(z["dlv3p/fp_masks"]).float()
    masks = [p.view(2 * d["B"], -1).to(dev) for p in flat.split([2 * d["B"] * 768, 2 * d["B"] * 512])]
    return model, dict(cfg, conf_thresh=d["conf_thresh"]), to_dev(batch, dev), masks


@functools.lru_cache(None)
def _dlv3p_state(shapes, seed):
    z = golden()[0]
    sd = seeded_state(list(shapes), seed)
    chk = np.array([sum(v.double().sum().item() for v in sd.values()), sum(v.double().abs().sum().item() for v in sd.values())])
    assert np.allclose(chk, z["dlv3p/w_checksum"], rtol=1e-9, atol=1e-6), "seeded weight stream differs from the fixture's"
    return sd


def grads_of(model):
    return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def zero_grads(model):
    for p in model.parameters():
        p.grad = None


def check_grads(z, pre, grads, full_names, log):
    assert sorted(grads) == [str(s) for s in z[pre + "grad_names"]]
    worst_n = worst_f = 0.0
    for k, g in grads.items():
        ref = z[pre + "gnorm/" + k]
        floor = 1e-5 if k == "decode_head.head.bias" else 1e-7     # (sum(softmax - onehot) ~ 0: cancellation noise)
        if ref[0] > 1e-4:
            worst_n = max(worst_n, abs(g.norm().item() - ref[0]) / ref[0])
        assert abs(g.norm().item() - ref[0]) < NORM_TOL * ref[0] + floor, f"{pre} grad norm of {k}: {g.norm().item()} vs {ref[0]}"
    for k in full_names:
        full = z[pre + "grad/" + k]
        e = np.abs(g_np(grads[k]) - full).max() / max(np.abs(full).max(), 1e-5)
        worst_f = max(worst_f, e)
        assert e < GRAD_TOL, f"{pre} grad of {k}: rel max err {e}"
    log.append(f"gradient norms worst rel {worst_n:.2e} (limit {NORM_TOL:.0e}), full gradients worst rel max {worst_f:.2e} "
               f"(limit {GRAD_TOL:.0e})")


def g_np(t):
    return t.detach().double().cpu().numpy()


def check_stats(z, pre, head, nbt, log):
    worst = 0.0
    for k, b in head.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == nbt == int(z[pre + "stat/" + k]), (k, int(b))
        else:
            e = np.abs(g_np(b) - z[pre + "stat/" + k]).max()
            worst = max(worst, e)
            assert e < STAT_TOL, f"{pre} {k}: {e}"
    log.append(f"running statistics max |d| {worst:.2e} (limit {STAT_TOL:.0e})")


def unpack_tie(z, key, shape):
    return np.unpackbits(z[key])[:int(np.prod(shape))].astype(bool).reshape(shape)


# ------------------------------------------------------------------------------------------------ 1. the rows as written
@pytest.mark.parametrize("model_name", [VLG, FT, FTAP])
def test_rows_as_written_take_a_step(dev, tmp_path, monkeypatch, model_name):
    """Each buildable `clip_encoder: null` row with ITS OWN clip_encoder / maskclip_consistency_lambda / mcc_loss_reduce:
    a semivl_train_step at crop 64, 5 classes, B = 2; then the optimizer its dict builds, GradAllReducer and a checkpoint."""
    from semivl_amd.checkpoint import load_checkpoint, save_checkpoint
    from semivl_amd.optim import optimizer_from_cfg
    from semivl_amd.synthetic import synthetic_batch
    from semivl_amd.train import GradAllReducer, semivl_train_step
    B, S_, N = 2, 64, 5
    model, cfg = tiny_row_model(tmp_path, monkeypatch, dev, model_name, S_, N)
    assert cfg["clip_encoder"] is None and cfg["maskclip_consistency_lambda"] == 0 and cfg["mcc_loss_reduce"] == "mean"
    assert model.clip_encoder is None and not any("clip_encoder" in k for k in model.state_dict())
    cfg = dict(cfg, conf_thresh=0.05)              # (random initialisation: the row's 0.95 would switch the unlabelled branches off)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    masks = row_fp_masks(model_name, B, dev)
    runs = []
    for _ in range(2):
        model.load_state_dict(state)
        zero_grads(model)
        losses, aux = semivl_train_step(model, synthetic_batch(B, S_, N, seed=99, device=dev), 1, 10, cfg,
                                        fp_masks=[m.clone() for m in masks], return_aux=True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(losses).all()), losses
        assert losses[5:8].tolist() == [0.0, 0.0, 0.0]
        assert all(float(v) > 0 for v in losses[:5]), losses
        assert aux["mclip"] is None and aux["mclip_other"] is None
        for n_, p in model.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n_
            else:
                assert p.grad is None, n_
        runs.append((losses.clone(), grads_of(model)))
    assert torch.equal(runs[0][0], runs[1][0])
    for n_ in runs[0][1]:
        assert torch.equal(runs[0][1][n_], runs[1][1][n_]), n_
    # optimizer / reducer / checkpoint as they are
    model.load_state_dict(state)
    zero_grads(model)
    opt = optimizer_from_cfg(model, cfg)
    assert opt.groups and not any("clip_encoder" in g_["name"] for g_ in opt.groups)
    red = GradAllReducer(opt)
    probe = next(p for n_, p in model.named_parameters() if n_.startswith("decode_head.") and p.requires_grad)
    before = probe.detach().clone()
    losses = semivl_train_step(model, synthetic_batch(B, S_, N, seed=99, device=dev), 1, 10, cfg, optimizer=opt, reducer=red,
                               fp_masks=[m.clone() for m in masks])
    torch.cuda.synchronize()
    assert torch.equal(losses, runs[0][0]) and not torch.equal(probe.detach(), before)
    ck = save_checkpoint(str(tmp_path / "latest.pth"), model, opt, 0)
    assert not any("clip_encoder" in k for k in ck["model"])
    assert not any("clip_encoder" in n_ for n_ in ck["optimizer"]["names"])
    after = {k: v.clone() for k, v in model.state_dict().items()}
    model.load_state_dict(state)
    assert load_checkpoint(str(tmp_path / "latest.pth"), model, strict=True) == 0
    for k, v in model.state_dict().items():
        assert torch.equal(v, after[k]), k
    opt.load_state_dict(torch.load(str(tmp_path / "latest.pth"), map_location="cpu")["optimizer"])


# ------------------------------------------------------------------------------------------------ 2. against the fixture
@pytest.mark.parametrize("mode", [0, 6])
def test_case_a_vlg_row_unguided_step(dev, mode):
    from semivl_amd import ops
    from semivl_amd.train import LOSS_NAMES, semivl_train_step
    z, c, _ = golden()
    log = []
    ops.set_gemm_emulation(mode)
    try:
        hip, _, batch, masks = vlg_case(dev)
        losses, aux = semivl_train_step(hip, batch, 1, 10, vlg_cfg(), fp_masks=masks, return_aux=True)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_emulation(0)
    losses = losses.cpu().numpy()
    for i, k in enumerate(LOSS_NAMES[:5]):
        ref = float(z["A/" + k])
        log.append(f"{k} {losses[i]:.7f} (float64 reference {ref:.7f}, |d| {abs(losses[i] - ref):.2e}, limit {LOSS_TOL:.0e})")
        assert abs(losses[i] - ref) < LOSS_TOL * max(1.0, abs(ref)), (k, losses[i], ref)
    assert losses[5:8].tolist() == [0.0, 0.0, 0.0]
    for k in ("mask_w", "mask_w_other"):
        ref = z["A/" + k]
        n = assert_labels(aux[k].cpu().numpy().astype(np.uint8), ref, unpack_tie(z, "A/tie/" + k, ref.shape), k)
        log.append(f"{k}: {n} pixels differ (all on ties)")
    check_grads(z, "A/", grads_of(hip), R.GRAD_FULL, log)
    print(f"\n[noguidance case A mode {mode}]\n  " + "\n  ".join(log))


@pytest.mark.parametrize("mode", [0, 6])
def test_case_b_dlv3p_row_unguided_step(dev, tmp_path, monkeypatch, mode):
    from semivl_amd import ops
    from semivl_amd.train import LOSS_NAMES, semivl_train_step
    z = golden()[0]
    log = []
    ops.set_gemm_emulation(mode)
    try:
        model, cfg, batch, masks = dlv3p_case(tmp_path, monkeypatch, dev)
        losses, aux = semivl_train_step(model, batch, 1, 10, cfg, fp_masks=masks, return_aux=True)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_emulation(0)
    losses = losses.cpu().numpy()
    for i, k in enumerate(LOSS_NAMES[:5]):
        ref = float(z["B/" + k])
        log.append(f"{k} {losses[i]:.7f} (float64 reference {ref:.7f}, |d| {abs(losses[i] - ref):.2e}, limit {LOSS_TOL:.0e})")
        assert abs(losses[i] - ref) < LOSS_TOL * max(1.0, abs(ref)), (k, losses[i], ref)
    assert losses[5:8].tolist() == [0.0, 0.0, 0.0]
    for k in ("mask_w", "mask_w_other"):
        ref = z["B/" + k]
        n = assert_labels(aux[k].cpu().numpy().astype(np.uint8), ref, unpack_tie(z, "B/tie/" + k, ref.shape), k)
        log.append(f"{k}: {n} pixels differ (all on ties)")
    check_grads(z, "B/", grads_of(model), R.GRAD_FULL_DLV3P, log)
    check_stats(z, "B/", model.decode_head, 2, log)
    print(f"\n[noguidance case B mode {mode}]\n  " + "\n  ".join(log))


# ------------------------------------------------------------------------------------------------ 3. skipping is real
def test_lambda_zero_never_touches_the_encoder(dev, monkeypatch):
    """A model WITH a clip encoder whose forward_tokens, and VLM.forward_maskclip, raise: lambda = 0 steps cleanly, and its
    losses[0:5] and every gradient equal those of the clip_encoder=None model with the same weights, bit for bit."""
    from semivl_amd.model.builder import VLM
    from semivl_amd.train import semivl_train_step
    z, c, _ = golden()
    plain, sd, batch, masks = vlg_case(dev)
    l0 = semivl_train_step(plain, {k: v.clone() for k, v in batch.items()}, 1, 10, vlg_cfg(), fp_masks=masks)
    g0 = grads_of(plain)
    with_enc = build_hip(c)
    assert with_enc.clip_encoder is not None
    res = with_enc.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith("clip_encoder.") for k in res.missing_keys)
    with_enc.to(dev)

    def boom(*a, **k):
        raise AssertionError("the guidance encoder was run although maskclip_consistency_lambda == 0")
    monkeypatch.setattr(with_enc.clip_encoder, "forward_tokens", boom)
    monkeypatch.setattr(VLM, "forward_maskclip", boom)
    l1, aux = semivl_train_step(with_enc, {k: v.clone() for k, v in batch.items()}, 1, 10, vlg_cfg(), fp_masks=masks,
                                return_aux=True)
    torch.cuda.synchronize()
    assert aux["mclip"] is None and aux["mclip_other"] is None
    assert torch.equal(l0[:5], l1[:5]) and l1[5:8].tolist() == [0.0, 0.0, 0.0]
    g1 = grads_of(with_enc)
    assert sorted(g0) == sorted(g1) and not any(k.startswith("clip_encoder.") for k in g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    with pytest.raises(AssertionError, match="guidance encoder was run"):       # (the guided default does call it)
        semivl_train_step(with_enc, {k: v.clone() for k, v in batch.items()}, 1, 10,
                          vlg_cfg(maskclip_consistency_lambda=[0.1, 0]), fp_masks=masks)


# ------------------------------------------------------------------------------------------------ 4. the 0 / 0 trap
def test_every_reduction_is_finite_and_identical_without_guidance(dev):
    """`mcc_loss_reduce='mean'` normalises by the number of labelled guidance pixels -- 0 without guidance: 0 * (x / 0)."""
    from semivl_amd.train import semivl_train_step
    hip, sd, batch, masks = vlg_case(dev)
    out = []
    for red in ("mean", "mean_valid", "mean_all"):
        zero_grads(hip)
        losses = semivl_train_step(hip, {k: v.clone() for k, v in batch.items()}, 1, 10, vlg_cfg(mcc_loss_reduce=red),
                                   fp_masks=masks)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(losses).all()), (red, losses)
        g = grads_of(hip)
        assert all(bool(torch.isfinite(v).all()) for v in g.values()), red
        out.append((losses.clone(), g))
    for losses, g in out[1:]:
        assert torch.equal(losses, out[0][0])
        for k in g:
            assert torch.equal(g[k], out[0][1][k]), k
    with pytest.raises(ValueError):             # still validated
        semivl_train_step(hip, {k: v.clone() for k, v in batch.items()}, 1, 10, vlg_cfg(mcc_loss_reduce="sum"), fp_masks=masks)


# ------------------------------------------------------------------------------------------------ 5. the refusal
def test_guided_cfg_on_a_model_without_encoder_is_refused_untouched(dev, tmp_path, monkeypatch):
    from semivl_amd.synthetic import synthetic_batch
    from semivl_amd.train import semivl_train_step
    model, cfg = tiny_row_model(tmp_path, monkeypatch, dev, FTAP)
    batch = synthetic_batch(2, 64, 5, seed=99, device=dev)
    img_s1 = batch["img_s1"].clone()
    assert bool(batch["mix1"].any())               # (the in-place CutMix of img_s1 would change it)
    state = {k: v.clone() for k, v in model.state_dict().items()}

    class NoReducer:
        def begin(self):
            raise AssertionError("reducer.begin() ran before the refusal")
    with pytest.raises(ValueError, match="maskclip_consistency_lambda.*clip_encoder"):
        semivl_train_step(model, batch, 1, 10, dict(cfg, maskclip_consistency_lambda=[0.1, 0]), reducer=NoReducer())
    torch.cuda.synchronize()
    assert torch.equal(batch["img_s1"], img_s1)
    for k, v in model.state_dict().items():        # weights and BatchNorm buffers (num_batches_tracked included)
        assert torch.equal(v, state[k]), k
    assert all(p.grad is None for p in model.parameters())
    with pytest.raises(RuntimeError, match="clip_encoder"):
        model.forward_maskclip(batch["img_w"], 0.9)


# ------------------------------------------------------------------------------------------------ 6. supervised_train_step
@pytest.mark.parametrize("mode", [0, 6])
def test_case_c_supervised_step_vlg(dev, mode):
    from semivl_amd import ops
    from semivl_amd.train import supervised_train_step
    z = golden()[0]
    log = []
    ops.set_gemm_emulation(mode)
    try:
        hip, _, batch, _ = vlg_case(dev)
        sup = dict(img_x=batch["img_x"], mask_x=batch["mask_x"])
        loss, aux = supervised_train_step(hip, sup, 1, 10, vlg_cfg(criterion=dict(name="CELoss", kwargs=dict(ignore_index=255))),
                                          return_aux=True)
        torch.cuda.synchronize()
        g = grads_of(hip)
        zero_grads(hip)
        loss2 = supervised_train_step(hip, sup, 1, 10, vlg_cfg())
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_emulation(0)
    assert tuple(loss.shape) == (1,) and loss.is_cuda and aux["upsample_in_loss"] and aux["mask_x_ohem"] is None
    assert tuple(aux["pred_x"].shape) == (batch["img_x"].shape[0], 21) + tuple(batch["img_x"].shape[2:])
    ref = float(z["C/loss"])
    log.append(f"loss {loss.item():.7f} (float64 reference {ref:.7f}, |d| {abs(loss.item() - ref):.2e}, limit {LOSS_TOL:.0e})")
    assert abs(loss.item() - ref) < LOSS_TOL * max(1.0, abs(ref))
    check_grads(z, "C/", g, R.GRAD_FULL, log)
    assert torch.equal(loss, loss2)                  # two runs, bit-equal
    for k, v in grads_of(hip).items():
        assert torch.equal(v, g[k]), k
    print(f"\n[noguidance case C mode {mode}]\n  " + "\n  ".join(log))


@pytest.mark.parametrize("mode", [0, 6])
def test_case_d_supervised_step_dlv3p_ohem(dev, tmp_path, monkeypatch, mode):
    from semivl_amd import ops
    from semivl_amd.train import ProbOhemCrossEntropy2d, supervised_train_step
    z, _, d = golden()
    log = []
    ops.set_gemm_emulation(mode)
    try:
        model, cfg, batch, _ = dlv3p_case(tmp_path, monkeypatch, dev)
        cfg = dict(cfg, criterion=d["criterion"])
        state = {k: v.clone() for k, v in model.state_dict().items()}
        sup = dict(img_x=batch["img_x"], mask_x=batch["mask_x"])
        loss, aux = supervised_train_step(model, sup, 1, 10, cfg, return_aux=True)
        torch.cuda.synchronize()
        g = grads_of(model)
        check_stats(z, "D/", model.decode_head, 1, log)      # ONE train-mode forward
        model.load_state_dict(state)
        zero_grads(model)
        loss2 = supervised_train_step(model, sup, 1, 10, cfg)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_emulation(0)
    assert not aux["upsample_in_loss"]               # the DeepLabV3+ head takes the resized path
    assert np.array_equal(aux["mask_x_ohem"].cpu().numpy().astype(np.uint8), z["D/mask_x_ohem"])
    crit = ProbOhemCrossEntropy2d(**d["criterion"]["kwargs"])
    assert torch.equal(aux["mask_x_ohem"], crit.relabel(aux["pred_x"], batch["mask_x"]))
    assert tuple(aux["dlogits"].shape) == tuple(aux["pred_x"].shape)
    ref = float(z["D/loss"])
    log.append(f"loss {loss.item():.7f} (float64 reference {ref:.7f}, |d| {abs(loss.item() - ref):.2e}, limit {LOSS_TOL:.0e})")
    assert abs(loss.item() - ref) < LOSS_TOL * max(1.0, abs(ref))
    check_grads(z, "D/", g, R.GRAD_FULL_DLV3P, log)
    assert torch.equal(loss, loss2)
    for k, v in grads_of(model).items():
        assert torch.equal(v, g[k]), k
    print(f"\n[noguidance case D mode {mode}]\n  " + "\n  ".join(log))


@pytest.mark.parametrize("kind", ["adamw", "sgd_original"])
def test_supervised_step_drives_the_fused_optimizers(dev, tmp_path, monkeypatch, kind):
    """zero_grad, backward, step, then poly_lr(iters, total_iters) with NO warm-up and NO scheduler_max_iters
    (supervised.py:294-300 ignores both even when the cfg carries them); one train-mode forward for BatchNorm."""
    from semivl_amd.optim import optimizer_from_cfg
    from semivl_amd.synthetic import synthetic_batch
    from semivl_amd.train import GradAllReducer, supervised_train_step
    model, cfg = tiny_row_model(tmp_path, monkeypatch, dev, FTAP)
    cfg = dict(cfg, warmup_iters=5, scheduler_max_iters=1000)
    if kind == "sgd_original":
        cfg.pop("optimizer")
        cfg.update(lr=0.001, lr_multi=10.0)
    opt = optimizer_from_cfg(model, cfg)
    red = GradAllReducer(opt)
    b = synthetic_batch(2, 64, 5, seed=99, device=dev)
    before = {k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
    k_it, total = 2, 10
    loss = supervised_train_step(model, dict(img_x=b["img_x"], mask_x=b["mask_x"]), k_it, total, cfg, optimizer=opt, reducer=red)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and float(loss) > 0
    moved = [k for k, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[k])]
    assert len(moved) == len(before), sorted(set(before) - set(moved))[:5]
    f = (1 - k_it / total) ** 0.9
    for g_ in opt.groups:
        assert g_["lr"] == pytest.approx(g_["initial_lr"] * f, rel=1e-12), g_["name"]
    for n_, buf in model.decode_head.named_buffers():
        if n_.endswith("num_batches_tracked"):
            assert int(buf) == 1, n_


@pytest.mark.parametrize("which", ["vlg", "dlv3p"])
def test_supervised_step_restores_its_overrides(dev, tmp_path, monkeypatch, which):
    from semivl_amd import ops
    from semivl_amd.train import supervised_train_step
    if which == "vlg":
        model, _, batch, _ = vlg_case(dev)
        cfg = vlg_cfg()
    else:
        model, cfg, batch, _ = dlv3p_case(tmp_path, monkeypatch, dev)
    head = model.decode_head
    head.act_limit_bytes = 12345
    keep = (head.remat, head.chunk_class_images, head.act_limit_bytes, ops.WGRAD_STREAM)
    cfg = dict(cfg, wgrad_stream=False, head_remat=1, head_chunk_class_images=7, act_mem_fraction=0.5)
    ops.WGRAD_STREAM = True
    try:
        sup = dict(img_x=batch["img_x"], mask_x=batch["mask_x"])
        loss = supervised_train_step(model, sup, 1, 10, cfg)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all())
        assert (head.remat, head.chunk_class_images, head.act_limit_bytes) == keep[:3] and ops.WGRAD_STREAM is True
        assert head._bwd_ranges is None and head._remat_step is None and head._live_class_images is None
        zero_grads(model)
        with pytest.raises(ValueError, match="mask_x"):       # a label map of the wrong shape: refused, nothing left behind
            supervised_train_step(model, dict(img_x=batch["img_x"], mask_x=batch["mask_x"][:, :-1].contiguous()), 1, 10, cfg)
        assert (head.remat, head.chunk_class_images, head.act_limit_bytes) == keep[:3] and ops.WGRAD_STREAM is True
        assert head._bwd_ranges is None and head._remat_step is None and head._live_class_images is None
        assert all(p.grad is None for p in model.parameters())
    finally:
        ops.WGRAD_STREAM = keep[3]


def test_supervised_loss_and_gradients_equal_autograd_through_the_model(dev):
    """The same model through `model(img)` + torch's own cross entropy and autograd (the full-resolution path): the step's
    device-side mean and its head-resolution gradient give the same loss and gradients."""
    import torch.nn.functional as F
    from semivl_amd.train import supervised_train_step
    hip, _, batch, _ = vlg_case(dev)
    loss = supervised_train_step(hip, dict(img_x=batch["img_x"], mask_x=batch["mask_x"]), 1, 10, vlg_cfg())
    g = grads_of(hip)
    zero_grads(hip)
    hip.train()
    ref = F.cross_entropy(hip(batch["img_x"]), batch["mask_x"], ignore_index=255)
    ref.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - ref.item()) < LOSS_TOL * max(1.0, abs(ref.item()))
    for k, v in grads_of(hip).items():
        e = (g[k] - v).abs().max().item() / max(v.abs().max().item(), 1e-3 if k == "decode_head.head.bias" else 1e-5)
        assert e < GRAD_TOL, (k, e)


# ------------------------------------------------------------------------------------------------ 7. the normaliser
@pytest.mark.parametrize("count", [1, 2, 3, 2 ** 31 + 1])
def test_inv_count_is_the_correctly_rounded_float(dev, count):
    from semivl_amd import ops
    c = torch.tensor([count], dtype=torch.int64, device=dev)
    out = torch.full((2,), -7.0, device=dev)
    ops.inv_count(c, out)
    torch.cuda.synchronize()
    want = np.float32(np.float64(1.0) / np.float64(count))
    assert np.float32(out[0].item()) == want, (out[0].item(), want)
    assert out[1].item() == -7.0                    # 1 float from 1 count: nothing else is written
