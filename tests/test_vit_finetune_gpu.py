"""Training the CLIP ViT beyond its attention projections (model_args=dict(freeze_backbone=False), wider exclude_keys):
the weight-gradient GEMMs on B-operand producers (gelu of the saved pre-activation, LayerNorm from the saved statistics,
the transposed patch matrix of the image) against float64, and the product step against the reference fixture and the
oracle."""
import copy

import numpy as np
import pytest
import torch

from golden_util import (MCC_TEXT, TEXT, build_oracle, fixture_batch, fixture_fp_masks, fixture_state, load_fixture,
                         seeded_state)

pytestmark = pytest.mark.gpu

CFG = dict(conf_thresh=0.95, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
           maskclip_consistency_lambda=[0.1, 0])


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))


def _run_modes(fn, ref64):
    """-> {mode: relative Frobenius distance from the float64 product}"""
    from semivl_amd import ops
    out = {}
    for mode in (0, 6):
        ops.set_gemm_emulation(mode)
        try:
            got = fn()
        finally:
            ops.set_gemm_emulation(0)
        torch.cuda.synchronize()
        assert torch.isfinite(got).all(), mode
        out[mode] = ((got.double() - ref64).norm() / ref64.norm()).item()
    return out


def _gate(errs):
    assert errs[0] < 1e-5, errs
    assert errs[6] <= 1.2 * errs[0], errs      # the per-kernel gate of the split arithmetic


@pytest.mark.parametrize("K", [4096, 2101])
def test_gelu_producer_matches_fp64(dev, K):
    from semivl_amd import ops
    g = torch.Generator(device=dev).manual_seed(K)
    a = torch.randn(K, 768, device=dev, generator=g)
    h = 2.0 * torch.randn(K, 3072, device=dev, generator=g)
    ref = a.double().t() @ _gelu64(h.double())
    _gate(_run_modes(lambda: ops.matmul_tn_gelu(a, h), ref))


@pytest.mark.parametrize("K", [4096, 2101])
def test_layernorm_producer_matches_fp64(dev, K):
    """With one large-magnitude row and a large gamma entry: LN output max (~1e4) far above the raw input's, so a
    fp16 x 2 scale taken from the raw input would overflow; the maximum pass must see the transformed operand."""
    from semivl_amd import ops
    g = torch.Generator(device=dev).manual_seed(K + 1)
    a = torch.randn(K, 3072, device=dev, generator=g)
    x = torch.randn(K, 768, device=dev, generator=g) + 0.3
    x[7] *= 50.0
    gamma = 1.0 + 0.1 * torch.randn(768, device=dev, generator=g)
    gamma[5] = 3000.0
    beta = 0.02 * torch.randn(768, device=dev, generator=g)
    _, st = ops.layernorm_fwd(x, gamma, beta, 1e-6)
    x64 = x.double()
    y64 = (x64 - x64.mean(1, keepdim=True)) / torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + 1e-6)
    y64 = y64 * gamma.double() + beta.double()
    # a scale from the raw input's maximum (max * 2^-e in [2^14, 2^15)) would put this operand above fp16's 65504
    assert y64.abs().max().item() > 16.0 * x.abs().max().item()
    ref = a.double().t() @ y64
    _gate(_run_modes(lambda: ops.matmul_tn_ln(a, x, st, gamma, beta), ref))


@pytest.mark.parametrize("S", [512, 801])
def test_patch_producer_matches_fp64(dev, S):
    """801 -> a 51 x 51 grid with the bottom / right zero fill (mmseg PatchEmbed padding='corner')."""
    import torch.nn.functional as F
    from semivl_amd import ops
    g = torch.Generator(device=dev).manual_seed(S)
    img = torch.randn(2, 3, S, S, device=dev, generator=g)
    hp = (S + 15) // 16
    a = torch.randn(2 * hp * hp, 768, device=dev, generator=g)
    pad = F.pad(img.double(), (0, hp * 16 - S, 0, hp * 16 - S))
    patches = F.unfold(pad, 16, stride=16).transpose(1, 2).reshape(2 * hp * hp, 768)   # k = (c, i, j)
    ref = a.double().t() @ patches
    _gate(_run_modes(lambda: ops.matmul_tn_patch(a, img, 16), ref))


def build_hip_ft(c, **model_args):
    """The product model at the fixture's dimensions with `model_args` merged into the model config (build_model's
    cfg['model_args'])."""
    from semivl_amd.model.builder import VLM, builtin_model_cfg
    mcfg = copy.deepcopy(builtin_model_cfg("vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb"))["model"]
    ccfg = copy.deepcopy(builtin_model_cfg("mcvit16"))["backbone"]
    S = c["S"]
    for bb in (mcfg["backbone"], ccfg):
        bb.update(img_size=(S, S), embed_dims=c["embed"], num_layers=c["layers"], num_heads=c["heads"])
        bb.pop("pretrained", None)
    mcfg["backbone"]["out_indices"] = c["out_indices"]
    mcfg["decode_head"].update(img_size=S, num_classes=21, text_channels=c["text_channels"], up_channels=c["up"],
                               skip_in_channels=(c["embed"], c["embed"]), skip_channels=c["skip"],
                               num_heads=c["dec_heads"], channels=c["channels"])
    mcfg.pop("type")
    mcfg.pop("pretrained", None)
    mcfg.update(model_args)
    return VLM(load_text_embedding=TEXT, load_mcc_text_embedding=MCC_TEXT, load_pl_text_embedding=TEXT,
               clip_encoder=ccfg, maskclip_class_filter=None, **mcfg)


def _step(hip, z, c, dev):
    from semivl_amd.train import LOSS_NAMES, semivl_train_step
    batch = {k: v.to(dev) for k, v in fixture_batch(z, c).items()}
    masks = [m.to(dev) for m in fixture_fp_masks(z, c)]
    iters, total = [int(v) for v in z["iters"]]
    hip.train()
    losses, _ = semivl_train_step(hip, batch, iters, total, dict(CFG, conf_thresh=c["conf_thresh"]), fp_masks=masks,
                                  return_aux=True)
    return dict(zip(LOSS_NAMES, losses.cpu().numpy()))


def test_finetune_step_matches_reference_fixture(dev):
    """freeze_backbone=False: every backbone tensor gets its gradient, same names, losses, norms and full gradients as the
    reference's own VLM (tests/golden/semivl_ft.npz) within test_model_gpu's tolerances."""
    z, c = load_fixture("ft")
    hip = build_hip_ft(c, freeze_backbone=False)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    hip.to(dev)
    losses = _step(hip, z, c, dev)
    for k, v in losses.items():
        assert abs(v - float(z[k])) < 1e-3 * max(1.0, abs(float(z[k]))), (k, v, float(z[k]))
    grads = {k: p.grad for k, p in hip.named_parameters() if p.grad is not None}
    assert sorted(grads) == [str(s) for s in z["grad_names"]]
    for k, g in grads.items():
        ref = z["gnorm/" + k]
        tol = 2e-3
        floor = 1e-5 if k == "decode_head.head.bias" else 1e-7
        assert abs(g.norm().item() - ref[0]) < tol * ref[0] + floor, f"grad norm of {k}: {g.norm().item()} vs {ref[0]}"
        if ("grad/" + k) in z.files:
            full = z["grad/" + k]
            e = np.abs(g.cpu().numpy() - full).max() / max(np.abs(full).max(), 1e-5)
            assert e < 5e-3, f"grad of {k}: rel max err {e}"


def test_subset_recipe_matches_oracle(dev):
    """exclude_keys=['attn', 'pos_embed', 'ln']: the LayerNorms train next to the attention, the FFNs, cls_token, patch
    embedding and proj stay without a gradient -- the same name set as the oracle's, the same norms."""
    from oracle import semivl_oracle as O
    z, c = load_fixture("tiny")
    keys = ["attn", "pos_embed", "ln"]
    hip = build_hip_ft(c, freeze_backbone=True, exclude_keys=keys)
    sd = fixture_state(z, c, hip)
    hip.load_state_dict(sd, strict=True)
    hip.to(dev)
    orc = build_oracle(c)
    orc.load_state_dict(sd, strict=True)
    for n, p in orc.backbone.named_parameters():
        p.requires_grad = any(k in n for k in keys)
    batch, masks = fixture_batch(z, c), fixture_fp_masks(z, c)
    iters, total = [int(v) for v in z["iters"]]
    loss, _ = O.semivl_step(orc, batch, iters, total, conf_thresh=c["conf_thresh"], fp_masks=masks)
    loss.backward()
    got = _step(hip, z, c, dev)
    assert abs(got["loss"] - loss.item()) < 1e-3
    og = {n: p.grad for n, p in orc.named_parameters() if p.grad is not None}
    hg = {n: p.grad for n, p in hip.named_parameters() if p.grad is not None}
    assert sorted(og) == sorted(hg), sorted(set(og) ^ set(hg))
    assert any(".ln1." in n for n in hg) and any(".ln2." in n for n in hg) and "backbone.ln0.weight" in hg
    assert not any(n.startswith("backbone.") and ".ffn." in n for n in hg) and "backbone.cls_token" not in hg and "backbone.proj.weight" not in hg
    for n, g in og.items():
        assert abs(hg[n].norm().item() - g.norm().item()) < 2e-3 * g.norm().item() + 1e-7, n


def test_fullsize_finetune_step_mode6_matches_oracle(dev):
    """One VOC step at 512^2, B = 2, freeze_backbone=False, split arithmetic (mode 6): every backbone gradient against the
    fp32 oracle with all backbone tensors trainable, per tensor (bounds of test_fullsize_gpu.py)."""
    from oracle import semivl_oracle as O
    from golden_util import PKG
    from semivl_amd import ops
    from semivl_amd.model.builder import build_model
    from semivl_amd.synthetic import exp40_cfg
    from semivl_amd.train import LOSS_NAMES, semivl_train_step
    import os
    torch.set_num_threads(min(32, torch.get_num_threads()))
    cfg = exp40_cfg(1, 512, 21, "pascal")
    cfg["model_args"] = dict(freeze_backbone=False)
    hip = build_model(cfg)
    sd = seeded_state([(k, tuple(v.shape)) for k, v in hip.state_dict().items()], 4242)
    hip.load_state_dict(sd, strict=True)
    hip.to(dev)
    t = torch.from_numpy(np.load(os.path.join(PKG, f"configs/_base_/datasets/text_embedding/voc12_wbg_{cfg['text_embedding_variant']}.npy")))
    mp = f"configs/_base_/datasets/text_embedding/voc12_wbg_{cfg['mcc_text']}.npy"
    m = torch.from_numpy(np.load(os.path.join(PKG, mp)))
    from semivl_amd.model.text_embeddings import get_class_to_concept_idxs
    orc = O.build_vlm(dict(nclass=21, crop=512), t, m, get_class_to_concept_idxs(mp) if m.shape[0] != 21 else None)
    orc.load_state_dict(sd, strict=True)
    for p in orc.backbone.parameters():
        p.requires_grad = True
    batch = O.synthetic_batch(2, 512, 21, seed=99)
    gm = torch.Generator().manual_seed(5)
    masks = [(torch.rand(4, ch, generator=gm) > 0.5).float() for ch in (768, 768, 512)]
    cfg = dict(cfg, conf_thresh=0.0)
    loss, _ = O.semivl_step(orc, batch, 100, 1000, conf_thresh=0.0, conf_mode=cfg["conf_mode"], fp_masks=masks)
    loss.backward()
    ops.set_gemm_emulation(6)
    try:
        losses, _ = semivl_train_step(hip, {k: v.to(dev) for k, v in batch.items()}, 100, 1000, cfg,
                                      fp_masks=[m_.to(dev) for m_ in masks], return_aux=True)
    finally:
        ops.set_gemm_emulation(0)
    assert abs(float(losses[0]) - loss.item()) < 1e-3
    og = {n: p.grad for n, p in orc.named_parameters() if p.grad is not None}
    hg = {n: p.grad for n, p in hip.named_parameters() if p.grad is not None}
    assert sorted(og) == sorted(hg), sorted(set(og) ^ set(hg))
    assert sum(n.startswith("backbone.") for n in hg) == sum(1 for _ in orc.backbone.parameters())
    fam = {}
    for n, g in og.items():
        if not n.startswith("backbone."):
            continue
        e = ((hg[n].cpu() - g).norm() / max(g.norm().item(), 1e-12)).item()
        f = next((k for k in ("attn", "ffn.layers.0", "ffn.layers.1", "ln1", "ln2", "ln0", "cls_token", "patch_embed",
                              "backbone.proj", "pos_embed") if k in n), "other")
        fam[f] = max(fam.get(f, 0.0), e)
        # far end of the chain (layer 0 and before): the cancellation amplification of test_fullsize_gpu.SHARED_FAR_END
        far = ".layers.0." in n or not n.startswith("backbone.layers.")
        assert e < (1.2e-2 if far else 4e-3), (n, e)
    print("worst mode-6 rel-L2 per backbone family:", {k: f"{v:.2e}" for k, v in sorted(fam.items())})
