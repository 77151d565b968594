"""Golden-vector generator for the LoRA recipes of the CLIP ViT (backbone=dict(..., lora_layers=[...]) with
exclude_keys=['lora'], model/backbone/lora.py).  Runs ONLY in the build container, like gen_golden_ft.py: it builds the
reference's own VLM with adapters in its MaskClipVisionTransformer at the 'tiny' fixture dimensions, drives one step of the
restated semivl.py:223-328 loop body with the reference's helpers and writes tests/golden/semivl_lora.npz in the
semivl_ft.npz layout (inputs and weights as seed checksums; losses, gradient names and norms, the full gradients of every
adapter tensor), one key prefix per case:

    A/  lora_layers=[0, 2], r=4, lora_scaling=2.0, targets 'qkvo', exclude_keys=['lora']: layer 0 runs both paths, layer 2
        is the v-only last block
    B/  lora_layers=[1], r=3, lora_scaling=0.5, targets 'qv', exclude_keys=['attn', 'pos_embed', 'lora']: the base
        projections train next to the adapters

The oracle has no adapters: the reference alone is the yardstick here.  The stored step is the reference's own code run in
FLOAT64 (parameters, inputs and the default dtype are float64, and the `.float()` casts inside the reference keep float64
for the duration of the run): its float32 run is printed next to it and lies further from its float64 run on the adapter
gradients of case B (5.5e-3 ... 9.1e-3 relative max, pure rounding: every label map and confidence decision of the two runs
is identical) than the 5e-3 the model test allows, so a float32 fixture would fail a product that computes the exact
gradient.  Weights, inputs and masks are the float32 seeded streams in both runs.

    python tests/golden/gen_golden_lora.py
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

CASES = {
    "A": dict(lora=dict(lora_layers=[0, 2], lora_r=4, lora_scaling=2.0, lora_dropout=0, lora_targets="qkvo"),
              exclude_keys=["lora"]),
    "B": dict(lora=dict(lora_layers=[1], lora_r=3, lora_scaling=0.5, lora_dropout=0, lora_targets="qv"),
              exclude_keys=["attn", "pos_embed", "lora"]),
}


def build_reference_lora(c, case):
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
    mcfg["backbone"].update(case["lora"])
    mcfg["decode_head"].update(img_size=S, num_classes=21, text_channels=c["text_channels"], up_channels=c["up"],
                               skip_in_channels=(c["embed"], c["embed"]), skip_channels=c["skip"],
                               num_heads=c["dec_heads"], channels=c["channels"])
    mcfg.pop("type")
    mcfg.pop("pretrained", None)
    mcfg.update(freeze_backbone=True, exclude_keys=case["exclude_keys"])
    mcfg["backbone"]["type"] = "MaskClipVisionTransformer"
    ccfg["type"] = "MaskClipVisionTransformer"
    mcfg["decode_head"]["type"] = "VLGHead"
    m = ref_vlm.VLM(load_text_embedding=G.TEXT, load_mcc_text_embedding=G.MCC_TEXT, load_pl_text_embedding=G.TEXT,
                    clip_encoder=ccfg, maskclip_class_filter=None, **mcfg)
    m.disable_dropout, m.fp_rate = True, 0.5
    m.forward = types.MethodType(forward_wrapper, m)
    # the layers' first-iteration self-check compares the adapted output with the base output: it holds for b_* = 0 only
    for lyr in m.backbone.layers:
        lyr.first_iter = False
    return m


def main():
    os.chdir(G.REF)
    sys.path.insert(0, G.REF)
    import _ref_shim
    _ref_shim.install()
    if not hasattr(F, "_scaled_dot_product_attention"):     # the private name lora.py:105 calls (torch < 2.0)
        F._scaled_dot_product_attention = lambda q, k, v: (F.scaled_dot_product_attention(q, k, v), None)
    from oracle import semivl_oracle as O
    import utils.train_utils as ref_tu
    import semivl as ref_semivl

    def ref_cwl(loss, conf, ign, conf_mode, conf_thresh):
        return ref_tu.confidence_weighted_loss(loss, conf, ign, dict(conf_mode=conf_mode, conf_thresh=conf_thresh))

    def ref_mc(pred, mask, ign, reduce):
        ref_semivl.mcc_loss_reduce = reduce
        ref_semivl.criterion_mc = (torch.nn.CrossEntropyLoss(ignore_index=255) if reduce == "mean" else
                                   torch.nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
        return ref_semivl.compute_mc_loss(pred, mask, ign)

    helpers = (ref_tu.cutmix_img_, ref_tu.cutmix_mask, ref_cwl, ref_mc)
    c = dict(G.CONFIGS["tiny"])
    B, S = c["B"], c["S"]
    batch = O.synthetic_batch(B, S, 21, seed=1234 + c["seed"])
    g = torch.Generator().manual_seed(c["seed"] + 100)
    fp_masks = [(torch.rand(2 * B, ch, generator=g) > 0.5).float() for ch in (c["embed"], c["embed"], 512)]
    iters, total = 10, 100

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

    out = dict(cfg=np.array(repr(dict(c, name="lora"))), iters=np.array([iters, total]),
               fp_masks=np.concatenate([m.numpy().ravel() for m in fp_masks]).astype(np.uint8),
               in_checksum=np.array([sum(v.double().sum().item() for v in batch.values())]))

    def run(case, sd, f64):
        """one step of the reference -> (loss, aux, grads); f64: in float64 (see the module docstring)"""
        to = (lambda t: t.double() if t.is_floating_point() else t) if f64 else (lambda t: t)
        keep = torch.Tensor.float
        if f64:
            torch.set_default_dtype(torch.float64)
            torch.Tensor.float = lambda self, *a, **k: self.double()
        try:
            torch.manual_seed(c["seed"])
            ref = build_reference_lora(c, case)
            ref.load_state_dict(sd, strict=True)
            assert all(p.dtype == (torch.float64 if f64 else torch.float32) for p in ref.parameters())
            masks = [to(m) for m in fp_masks]
            feeder, orig = G.MaskFeeder(masks), F.dropout2d
            F.dropout2d = feeder
            try:
                loss, aux = O.semivl_step(Adapter(ref), {k: to(v) for k, v in batch.items()}, iters, total,
                                          conf_thresh=c["conf_thresh"], fp_masks=masks, helpers=helpers)
            finally:
                F.dropout2d = orig
            loss.backward()
            assert loss.dtype == (torch.float64 if f64 else torch.float32)
            return loss.detach(), aux, {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
        finally:
            torch.Tensor.float = keep
            torch.set_default_dtype(torch.float32)

    for name, case in CASES.items():
        ref = build_reference_lora(c, case)
        sd = seeded_state([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], c["seed"])
        assert all(v.abs().max() > 0 for k, v in sd.items() if ".lora.b_" in k)
        l32, _, g32 = run(case, sd, False)
        loss, aux, rg = run(case, sd, True)
        assert set(g32) == set(rg)
        nl = [k for k in rg if ".lora." in k]
        gap = {k: ((g32[k].double() - rg[k]).abs().max() / rg[k].abs().max().clamp_min(1e-30)).item() for k in nl}
        print(f"[lora {name}] float32 run: loss {l32.item():.8f}; adapter gradients, rel max distance from the float64 run: "
              f"worst {max(gap.values()):.2e} ({max(gap, key=gap.get)})")
        loss, aux = loss.float(), {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in aux.items()}
        rg = {k: v.float() for k, v in rg.items()}
        print(f"[lora {name}] loss {loss.item():.8f}; {len(rg)} grads, {len(nl)} of them adapters, "
              f"{sum(k.startswith('backbone.') for k in rg)} backbone")
        # (the q / k adapters of the v-only last block reach the loss through zero gradients only: they get all-zero grads)
        zero = [k for k in nl if rg[k].abs().max() == 0]
        print(f"    all-zero adapter gradients: {zero}")
        assert nl and len(zero) < len(nl)
        pre = name + "/"
        out[pre + "case"] = np.array(repr(case))
        out[pre + "state_keys"] = np.array(list(sd))
        out[pre + "loss"] = loss.detach().numpy()
        for k in ("loss_x", "loss_s1", "loss_s2", "loss_fp", "loss_mc_s1", "loss_mc_s2", "loss_mc_fp"):
            out[pre + k] = aux[k].detach().numpy()
        out[pre + "grad_names"] = np.array(sorted(rg))
        out[pre + "w_checksum"] = np.array([sum(v.double().sum().item() for v in sd.values()),
                                            sum(v.double().abs().sum().item() for v in sd.values())])
        for k in sorted(rg):
            out[pre + "gnorm/" + k] = np.array([rg[k].norm().item(), rg[k].flatten()[0].item(), rg[k].flatten()[-1].item()])
        for k in nl:
            out[pre + "grad/" + k] = rg[k].numpy()
    path = os.path.join(HERE, "semivl_lora.npz")
    np.savez_compressed(path, **out)
    print(f"    wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB; semivl_ft.npz: "
          f"{os.path.getsize(os.path.join(HERE, 'semivl_ft.npz')) / 1e6:.2f} MB)")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "semivl_ft.npz"))


if __name__ == "__main__":
    main()
