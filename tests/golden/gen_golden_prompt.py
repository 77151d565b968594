"""Golden-vector generator for the deep visual prompts of the CLIP ViT (backbone=dict(..., num_prompt_tokens=P),
maskclip_vit.py:359-368,510-536).  Runs ONLY in the build container, like gen_golden_lora.py: it builds the reference's own
VLM with prompt tokens in its MaskClipVisionTransformer, drives one step of the restated semivl.py:223-328 loop body with the
reference's helpers and writes tests/golden/semivl_prompt.npz in the semivl_lora.npz layout (inputs and weights as seed
checksums; losses, gradient names and norms, the full gradients of the three prompt tensors), one key prefix per case:

    A/  the 'conf' fixture dimensions (embed 64, 3 layers, 1 head: head dim 64), num_prompt_tokens=5, exclude_keys=['prompt'],
        disable_dropout=True: 70 rows per image inside the blocks
    B/  the same with 4 heads (head dim 16), num_prompt_tokens=3, exclude_keys=['attn', 'pos_embed', 'prompt'],
        disable_dropout=False: prompt_dropout is live in the two train-mode forwards of the step

and per case the encoder alone: features of the backbone for the fixture's img_x (sample 0 stored; the 512-channel embedding
every 8th channel) and the prompt gradients of sum_j <feature_j, seeded cotangent_j>, in float64.

prompt_dropout is replaced by a recorder that draws seeded {0, 1} masks in train mode only, applies x * (mask / (1 - p)) like
nn.Dropout, and keeps the masks in call order (stored bit-packed).  With disable_dropout=True the recorder is switched off:
that is the behaviour the configs ask for.  (The reference's own forward_wrapper puts its nn.Dropout modules into eval mode
only AFTER extract_feat, builder.py:60-64, so its first train-mode forward after every model.train() still draws prompt
dropout; the product does not reproduce that.)

The stored step is the reference's own code run in FLOAT64, as for the LoRA fixture; its float32 run is printed next to it.
prompt_norm.* has grad None after the reference's backward: checked here and stored as a flag.

    python tests/golden/gen_golden_prompt.py
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
import gen_golden as G  # noqa: E402  (paths, seeds, the mask feeder, the fixture dimensions)
from golden_util import seeded_state, smooth_batch  # noqa: E402
from prompt_ref import PROMPT_KEYS, seeded_cots  # noqa: E402

CASES = {
    "A": dict(backbone=dict(num_prompt_tokens=5), exclude_keys=["prompt"], disable_dropout=True, cfg=dict(G.CONFIGS["conf"])),
    "B": dict(backbone=dict(num_prompt_tokens=3), exclude_keys=["attn", "pos_embed", "prompt"], disable_dropout=False,
              cfg=dict(G.CONFIGS["conf"], heads=4, seed=16)),
}


class Recorder(torch.nn.Module):
    """nn.Dropout(p) with seeded masks that are kept: live in train mode and when `enabled` only"""

    def __init__(self, p, enabled):
        super().__init__()
        self.p, self.enabled, self.gen, self.masks = p, enabled, torch.Generator(), []

    def reset(self, seed):
        self.gen.manual_seed(seed)
        self.masks = []

    def forward(self, x):
        if not (self.training and self.enabled):
            return x
        m = (torch.rand(x.shape, generator=self.gen, dtype=torch.float32) < 1.0 - self.p).float()   # one stream in both precisions
        self.masks.append(m)
        return x * (m.to(x.dtype) / (1.0 - self.p))


def build_reference_prompt(c, case):
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
    mcfg["backbone"].update(case["backbone"])
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
    m.disable_dropout, m.fp_rate = case["disable_dropout"], 0.5
    m.forward = types.MethodType(forward_wrapper, m)
    assert isinstance(m.backbone.prompt_dropout, torch.nn.Dropout) and m.backbone.prompt_dropout.p == 0.1
    m.backbone.prompt_dropout = Recorder(0.1, enabled=not case["disable_dropout"])
    assert not hasattr(m.clip_encoder, "deep_prompt_embeddings")
    return m


def pack_masks(masks):
    a = torch.stack(masks).numpy().astype(np.uint8)
    return np.packbits(a.ravel()), np.array(a.shape)


def main():
    os.chdir(G.REF)
    sys.path.insert(0, G.REF)
    import _ref_shim
    _ref_shim.install()
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

    out = dict(cfg=np.array(repr(dict(CASES["A"]["cfg"], name="prompt"))), iters=np.array([iters, total]))

    for name, case in CASES.items():
        c = case["cfg"]
        B, S = c["B"], c["S"]
        batch = O.synthetic_batch(B, S, 21, seed=1234 + c["seed"])
        if c.get("smooth_inputs"):
            batch = smooth_batch(batch)
        g = torch.Generator().manual_seed(c["seed"] + 100)
        fp_masks = [(torch.rand(2 * B, ch, generator=g) > 0.5).float() for ch in (c["embed"], c["embed"], 512)]
        conf_thresh = c["conf_thresh"]

        def run(sd, f64):
            """one step of the reference, then its encoder alone -> (loss, aux, grads, step masks, encoder results)"""
            to = (lambda t: t.double() if t.is_floating_point() else t) if f64 else (lambda t: t)
            keep = torch.Tensor.float
            if f64:
                torch.set_default_dtype(torch.float64)
                torch.Tensor.float = lambda self, *a, **k: self.double()
            try:
                torch.manual_seed(c["seed"])
                ref = build_reference_prompt(c, case)
                ref.load_state_dict(sd, strict=True)
                assert all(p.dtype == (torch.float64 if f64 else torch.float32) for p in ref.parameters())
                rec = ref.backbone.prompt_dropout
                rec.reset(c["seed"] + 200)
                masks = [to(m) for m in fp_masks]
                feeder, orig = G.MaskFeeder(masks), F.dropout2d
                F.dropout2d = feeder
                try:
                    loss, aux = O.semivl_step(Adapter(ref), {k: to(v) for k, v in batch.items()}, iters, total,
                                              conf_thresh=conf_thresh, fp_masks=masks, helpers=helpers)
                finally:
                    F.dropout2d = orig
                loss.backward()
                assert loss.dtype == (torch.float64 if f64 else torch.float32)
                grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
                norm_none = all(p.grad is None and p.requires_grad for k, p in ref.named_parameters() if ".prompt_norm." in k)
                step_masks = list(rec.masks)
                # the encoder alone, in train mode (the recorder is live where the case has dropout)
                for p in ref.parameters():
                    p.grad = None
                rec.reset(c["seed"] + 300)
                ref.train()
                feats, glob = ref.backbone(to(batch["img_x"]))
                feats = [f.flatten(2).transpose(1, 2) for f in feats]
                cots = seeded_cots([tuple(f.shape) for f in feats], c["seed"] + 400)
                sum((f * to(ct)).sum() for f, ct in zip(feats, cots)).backward()
                bb = dict(ref.backbone.named_parameters())
                enc = dict(feats=[f.detach() for f in feats], glob=glob.detach(), masks=list(rec.masks),
                           grads={k: bb[k].grad.detach().clone() for k in PROMPT_KEYS})
                return loss.detach(), aux, grads, norm_none, step_masks, enc
            finally:
                torch.Tensor.float = keep
                torch.set_default_dtype(torch.float32)

        ref = build_reference_prompt(c, case)
        sd = seeded_state([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], c["seed"], c.get("logit_gain"))
        l32, _, g32, none32, m32, e32 = run(sd, False)
        loss, aux, rg, norm_none, step_masks, enc = run(sd, True)
        assert set(g32) == set(rg) and norm_none and none32
        assert len(m32) == len(step_masks) and all(torch.equal(a, b) for a, b in zip(m32, step_masks))
        pk = ["backbone." + k for k in PROMPT_KEYS]
        assert all(k in rg for k in pk) and not any(".prompt_norm." in k for k in rg)

        def rel(a, b):
            return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()

        gap = {k: rel(g32[k], rg[k]) for k in pk}
        ngap = {k: abs(g32[k].double().norm().item() / rg[k].norm().item() - 1) for k in rg
                if rg[k].norm() > 0 and k != "decode_head.head.bias"}      # (that one sums to zero: its norm is rounding noise)
        print(f"[prompt {name}] float32 run: loss {l32.item():.8f} (float64 {loss.item():.8f}); prompt gradients, rel max distance "
              f"from the float64 run: worst {max(gap.values()):.2e} ({max(gap, key=gap.get)}); gradient norms: worst "
              f"{max(ngap.values()):.2e} ({max(ngap, key=ngap.get)})")
        egap = {k: rel(e32["grads"][k], enc["grads"][k]) for k in PROMPT_KEYS}
        print(f"[prompt {name}] encoder alone, float32 run: features {max(rel(a, b) for a, b in zip(e32['feats'], enc['feats'])):.2e}, "
              f"prompt gradients {max(egap.values()):.2e} from the float64 run")
        loss, aux = loss.float(), {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in aux.items()}
        rg = {k: v.float() for k, v in rg.items()}
        print(f"[prompt {name}] loss {loss.item():.8f}; {len(rg)} grads, {sum(k.startswith('backbone.') for k in rg)} backbone; "
              f"{len(step_masks)} step masks, {len(enc['masks'])} encoder masks; prompt_norm grads None: {norm_none}")
        pre = name + "/"
        spec = {k: v for k, v in case.items() if k != "cfg"}
        out[pre + "case"] = np.array(repr(spec))
        out[pre + "cfg"] = np.array(repr(dict(c, name="prompt")))
        out[pre + "state_keys"] = np.array(list(sd))
        out[pre + "fp_masks"] = np.concatenate([m.numpy().ravel() for m in fp_masks]).astype(np.uint8)
        out[pre + "in_checksum"] = np.array([sum(v.double().sum().item() for v in batch.values())])
        out[pre + "loss"] = loss.detach().numpy()
        for k in ("loss_x", "loss_s1", "loss_s2", "loss_fp", "loss_mc_s1", "loss_mc_s2", "loss_mc_fp"):
            out[pre + k] = aux[k].detach().numpy()
        out[pre + "grad_names"] = np.array(sorted(rg))
        out[pre + "prompt_norm_grad_is_none"] = np.array([norm_none])
        out[pre + "w_checksum"] = np.array([sum(v.double().sum().item() for v in sd.values()),
                                            sum(v.double().abs().sum().item() for v in sd.values())])
        for k in sorted(rg):
            out[pre + "gnorm/" + k] = np.array([rg[k].norm().item(), rg[k].flatten()[0].item(), rg[k].flatten()[-1].item()])
        for k in pk:
            out[pre + "grad/" + k] = rg[k].numpy()
        if step_masks:
            out[pre + "prompt_masks"], out[pre + "prompt_masks_shape"] = pack_masks(step_masks)
        if enc["masks"]:
            out[pre + "enc_masks"], out[pre + "enc_masks_shape"] = pack_masks(enc["masks"])
        for j, f in enumerate(enc["feats"]):
            out[pre + f"enc/feat{j}"] = (f[0, :, ::8] if f.shape[-1] == 512 else f[0]).numpy()
        out[pre + "enc/glob"] = enc["glob"].numpy()
        for k in PROMPT_KEYS:
            out[pre + "enc/grad/" + k] = enc["grads"][k].numpy()
    path = os.path.join(HERE, "semivl_prompt.npz")
    np.savez_compressed(path, **out)
    print(f"    wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB; dlv3p_head.npz: "
          f"{os.path.getsize(os.path.join(HERE, 'dlv3p_head.npz')) / 1e6:.2f} MB)")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "dlv3p_head.npz")) // 2


if __name__ == "__main__":
    main()
