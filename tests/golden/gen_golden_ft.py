"""Golden-vector generator for full fine-tuning of the CLIP ViT (model_args=dict(freeze_backbone=False): the `ft`
recipes, configs/_base_/models/vlm-dlv3p-bn12-sk4-ft-mcvitb.py / exp 41).  Runs ONLY in the build container, like
gen_golden.py: it builds the reference's own VLM from the VLG config with freeze_backbone=False at the 'tiny' fixture
dimensions, drives one step of the restated semivl.py:223-328 loop body with it, checks the oracle restatement (every
backbone tensor trainable) against it and writes tests/golden/semivl_ft.npz (inputs and weights as seed checksums; losses,
gradient names and norms, the full gradients of a few backbone tensors).

    python tests/golden/gen_golden_ft.py
"""
import os
import runpy
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (paths, seeds, the mask feeder, the 'tiny' dimensions)
from golden_util import seeded_state  # noqa: E402

FULL = ("backbone.layers.0.ffn.layers.0.0.weight", "backbone.layers.1.ln2.weight",
        "backbone.patch_embed.projection.weight", "backbone.cls_token", "backbone.proj.weight")


def build_reference_ft(c):
    import model.vlm as ref_vlm  # noqa: registers VLM
    import model.decode_heads.vlg_head  # noqa: registers VLGHead
    import third_party.maskclip.models.backbones.maskclip_vit  # noqa: registers the ViT
    from model.builder import forward_wrapper
    mcfg = runpy.run_path("configs/_base_/models/vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb.py")["model"]
    ccfg = runpy.run_path("configs/_base_/models/mcvit16.py")["backbone"]
    S = c["S"]
    for bb in (mcfg["backbone"], ccfg):
        bb.update(img_size=(S, S), embed_dims=c["embed"], num_layers=c["layers"], num_heads=c["heads"])
        bb.pop("pretrained", None)
        bb.pop("type", None)
    mcfg["backbone"]["out_indices"] = c["out_indices"]
    mcfg["decode_head"].update(img_size=S, num_classes=21, text_channels=c["text_channels"], up_channels=c["up"],
                               skip_in_channels=(c["embed"], c["embed"]), skip_channels=c["skip"],
                               num_heads=c["dec_heads"], channels=c["channels"])
    mcfg.pop("type")
    mcfg.pop("pretrained", None)
    mcfg["freeze_backbone"] = False          # what cfg['model_args'] = dict(freeze_backbone=False) sets
    mcfg["backbone"]["type"] = "MaskClipVisionTransformer"
    ccfg["type"] = "MaskClipVisionTransformer"
    mcfg["decode_head"]["type"] = "VLGHead"
    m = ref_vlm.VLM(load_text_embedding=G.TEXT, load_mcc_text_embedding=G.MCC_TEXT, load_pl_text_embedding=G.TEXT,
                    clip_encoder=ccfg, maskclip_class_filter=None, **mcfg)
    m.disable_dropout, m.fp_rate = True, 0.5
    m.forward = types.MethodType(forward_wrapper, m)
    return m


def main():
    os.chdir(G.REF)
    sys.path.insert(0, G.REF)
    import _ref_shim
    _ref_shim.install()
    from oracle import semivl_oracle as O
    from model.text_embeddings import get_class_to_concept_idxs
    import utils.train_utils as ref_tu
    import semivl as ref_semivl
    cls2con = get_class_to_concept_idxs(G.MCC_TEXT)

    def ref_cwl(loss, conf, ign, conf_mode, conf_thresh):
        return ref_tu.confidence_weighted_loss(loss, conf, ign, dict(conf_mode=conf_mode, conf_thresh=conf_thresh))

    def ref_mc(pred, mask, ign, reduce):
        ref_semivl.mcc_loss_reduce = reduce
        ref_semivl.criterion_mc = (torch.nn.CrossEntropyLoss(ignore_index=255) if reduce == "mean" else
                                   torch.nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
        return ref_semivl.compute_mc_loss(pred, mask, ign)

    helpers = (ref_tu.cutmix_img_, ref_tu.cutmix_mask, ref_cwl, ref_mc)
    text = torch.from_numpy(np.load(G.TEXT))
    mcc = torch.from_numpy(np.load(G.MCC_TEXT))
    c = dict(G.CONFIGS["tiny"])
    torch.manual_seed(c["seed"])
    ref = build_reference_ft(c)
    assert all(p.requires_grad for p in ref.backbone.parameters())
    sd = seeded_state([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], c["seed"])
    ref.load_state_dict(sd, strict=True)
    orc = O.build_vlm(dict(nclass=21, crop=c["S"], embed=c["embed"], layers=c["layers"], heads=c["heads"],
                           out_indices=tuple(c["out_indices"]), channels=c["channels"], text_channels=c["text_channels"],
                           up=c["up"], skip_in=(c["embed"], c["embed"]), skip=c["skip"]), text, mcc, cls2con)
    for lyr in orc.decode_head.layers:
        lyr.transformer.attn.attn.num_heads = c["dec_heads"]
    orc.load_state_dict(sd, strict=True)
    for p in orc.backbone.parameters():      # exclude_keys=("",): every backbone tensor trainable
        p.requires_grad = True
    B, S = c["B"], c["S"]
    batch = O.synthetic_batch(B, S, 21, seed=1234 + c["seed"])
    g = torch.Generator().manual_seed(c["seed"] + 100)
    fp_masks = [(torch.rand(2 * B, ch, generator=g) > 0.5).float() for ch in (c["embed"], c["embed"], 512)]
    iters, total = 10, 100

    def run(model, is_ref):
        model.zero_grad()
        if is_ref:
            feeder, orig = G.MaskFeeder(fp_masks), F.dropout2d
            F.dropout2d = feeder

            class Adapter:
                def __init__(s, m):
                    s.m = m

                def eval(s):
                    s.m.eval()

                def train(s):
                    s.m.train()

                def __call__(s, img, need_fp=False, fp_masks=None):
                    return s.m(img, need_fp=need_fp)

                def forward_maskclip(s, img, t):
                    return s.m.forward_maskclip(img, t)
            try:
                loss, aux = O.semivl_step(Adapter(model), batch, iters, total, conf_thresh=c["conf_thresh"],
                                          fp_masks=fp_masks, helpers=helpers)
            finally:
                F.dropout2d = orig
        else:
            loss, aux = O.semivl_step(model, batch, iters, total, conf_thresh=c["conf_thresh"], fp_masks=fp_masks)
        loss.backward()
        return loss.detach(), aux, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}

    rl, raux, rg = run(ref, True)
    ol, oaux, og = run(orc, False)
    print(f"[ft] loss ref {rl.item():.8f} oracle {ol.item():.8f}")
    assert abs(rl.item() - ol.item()) <= 1e-6 * max(1.0, abs(rl.item()))
    assert set(rg) == set(og), set(rg) ^ set(og)
    worst = max(((rg[k] - og[k]).abs().max() / (rg[k].abs().max() + 1e-12)).item() for k in rg)
    nb = sum(k.startswith("backbone.") for k in rg)
    print(f"    {len(rg)} grads ({nb} backbone), worst rel max-err oracle vs reference {worst:.2e}")
    assert worst < 1e-4
    out = dict(cfg=np.array(repr(dict(c, name="ft"))), iters=np.array([iters, total]), loss=rl.numpy(),
               **{k: raux[k].detach().numpy() for k in ("loss_x", "loss_s1", "loss_s2", "loss_fp", "loss_mc_s1",
                                                        "loss_mc_s2", "loss_mc_fp")},
               fp_masks=np.concatenate([m.numpy().ravel() for m in fp_masks]).astype(np.uint8),
               grad_names=np.array(sorted(rg)),
               w_checksum=np.array([sum(v.double().sum().item() for v in sd.values()),
                                    sum(v.double().abs().sum().item() for v in sd.values())]),
               in_checksum=np.array([sum(v.double().sum().item() for v in batch.values())]))
    for k in sorted(rg):
        out["gnorm/" + k] = np.array([rg[k].norm().item(), rg[k].flatten()[0].item(), rg[k].flatten()[-1].item()])
    for k in FULL:
        out["grad/" + k] = rg[k].numpy()
    path = os.path.join(HERE, "semivl_ft.npz")
    np.savez_compressed(path, **out)
    print(f"    wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
