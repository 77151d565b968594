"""Golden-vector generator for stochastic depth in the CLIP ViT (backbone=dict(..., drop_path_rate=r),
maskclip_vit.py:77-100,120-144,299-312).  Runs ONLY in the build container, like gen_golden_prompt.py: it builds the
reference's own VLM, drives one step of the restated semivl.py:223-328 loop body with the reference's helpers and writes
tests/golden/semivl_droppath.npz in the semivl_prompt.npz layout (inputs and weights as seed checksums; losses, gradient names
and norms, the full gradients of a few small tensors), one key prefix per case:

    A/  the 'conf' fixture dimensions (embed 64, 3 layers, 1 head: head dim 64), freeze_backbone=False (the `ft` recipe: every
        backbone tensor trains), drop_path_rate=0.5: rates 0, 0.25, 0.5
    B/  the same with 4 heads (head dim 16), lora_layers=[1, 2], num_prompt_tokens=3, exclude_keys=['attn', 'pos_embed', 'lora',
        'prompt'], drop_path_rate=0.4 (rates 0, 0.2, 0.4), disable_dropout=True: stochastic depth stays live, prompt dropout
        is off

and per case the encoder alone in train mode: features of the backbone for the fixture's img_x (sample 0 stored; the
512-channel embedding every 8th channel), the global embedding and the gradients of sum_j <feature_j, seeded cotangent_j> for
the case's `enc_keys`, in float64.

mmcv's DropPath is not in the reference tree; tests/golden/_ref_shim.py builds every block's attn.dropout_layer and
ffn.dropout_layer as nn.Identity.  After construction each is replaced by a recorder that applies x / keep * mask in train mode
(one seeded {0, 1} draw per sample, keep = 1 - dpr[layer], dpr the float32 linspace of the reference's constructor) and logs
(layer, module, mask) in call order.  A block's `ffn` module is called twice where the block returns q, k, v (v path first):
the log is stored as (train-mode forward, layer, site) with site 0 'attn', 1 'ffn', 2 'ffn_v'.  The mask seed is the first one
from the case's base seed whose draws give every site kind a kept and a dropped sample, one site with every sample dropped and
one with every sample kept, among the sites whose branch reaches an output (the last block's x path does not in the step);
this is asserted.  The blocks' first-iteration self-check (adapted against base attention output) would call the attention's
dropout_layer a second time with another draw: it is switched off, as in gen_golden_lora.py.  prompt_dropout is replaced by a
switched-off recorder as in gen_golden_prompt.py (disable_dropout=True).

The stored step is the reference's own code run in FLOAT64; its float32 run is printed next to it.

    python tests/golden/gen_golden_droppath.py
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
from droppath_ref import SITES, seeded_cots  # noqa: E402
from gen_golden_prompt import Recorder as PromptRecorder  # noqa: E402

CASES = {
    "A": dict(backbone=dict(drop_path_rate=0.5), model_args=dict(freeze_backbone=False), disable_dropout=True,
              cfg=dict(G.CONFIGS["conf"]),
              full=["backbone.cls_token", "backbone.ln0.weight", "backbone.layers.1.ln2.weight",
                    "backbone.layers.1.ffn.layers.0.0.bias", "backbone.layers.1.attn.attn.out_proj.bias",
                    "backbone.layers.2.ffn.layers.1.bias", "backbone.layers.2.attn.attn.out_proj.weight"],
              enc_keys=["cls_token", "layers.0.ln1.weight", "layers.1.ln2.bias", "layers.1.ffn.layers.1.bias",
                        "layers.1.attn.attn.out_proj.bias", "layers.1.attn.attn.in_proj_bias", "layers.2.ffn.layers.0.0.bias",
                        "layers.2.attn.attn.out_proj.weight"]),
    "B": dict(backbone=dict(drop_path_rate=0.4, num_prompt_tokens=3, lora_layers=[1, 2], lora_r=3, lora_scaling=0.5,
                            lora_dropout=0, lora_targets="qkvo"),
              model_args=dict(freeze_backbone=True, exclude_keys=["attn", "pos_embed", "lora", "prompt"]), disable_dropout=True,
              cfg=dict(G.CONFIGS["conf"], heads=4, seed=16),
              full=["backbone.deep_prompt_embeddings", "backbone.prompt_proj.weight", "backbone.prompt_proj.bias",
                    "backbone.layers.1.lora.b_o.weight", "backbone.layers.2.lora.a_v.weight",
                    "backbone.layers.1.attn.attn.in_proj_bias", "backbone.layers.2.attn.attn.out_proj.bias"],
              enc_keys=["deep_prompt_embeddings", "prompt_proj.weight", "prompt_proj.bias", "layers.1.lora.b_o.weight",
                        "layers.1.lora.a_q.weight", "layers.2.lora.a_v.weight", "layers.1.attn.attn.in_proj_bias",
                        "layers.2.attn.attn.out_proj.bias"]),
}


class Tape:
    """the draws of one run: call j's mask comes from its own generator (seed, j), so a seed can be judged by replaying the
    call log without running the model"""

    def __init__(self):
        self.seed, self.log = 0, []

    def reset(self, seed):
        self.seed, self.log = seed, []

    @staticmethod
    def draw(seed, j, n, keep):
        g = torch.Generator().manual_seed(seed * 4096 + j)
        return (torch.rand(n, generator=g, dtype=torch.float32) < keep).float()      # one stream in both precisions

    def mask(self, layer, kind, n, keep):
        m = self.draw(self.seed, len(self.log), n, keep)
        self.log.append((layer, kind, m))
        return m


class DropPathRecorder(torch.nn.Module):
    """DropPath(p) with seeded, kept masks: x / keep * mask[:, None, None] in train mode with p > 0, the identity otherwise"""

    def __init__(self, p, layer, kind, tape):
        super().__init__()
        self.p, self.layer, self.kind, self.tape = p, layer, kind, tape

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        keep = 1.0 - self.p
        m = self.tape.mask(self.layer, self.kind, x.shape[0], keep)
        return x / keep * m.to(x.dtype).view(-1, *([1] * (x.dim() - 1)))


def sited(log):
    """call log [(layer, 'attn' | 'ffn', mask)] -> [(forward, layer, site index, mask)] in call order"""
    out, fwd, prev, i = [], 0, -1, 0
    while i < len(log):
        layer = log[i][0]
        if layer <= prev:       # a block's calls come in one group per forward, blocks in ascending order
            fwd += 1
        prev = layer
        sites = ("ffn_v", "attn", "ffn") if log[i][1] == "ffn" else ("attn", "ffn")
        grp = log[i:i + len(sites)]
        assert [e[0] for e in grp] == [layer] * len(sites) and [e[1] for e in grp] == [s.split("_")[0] for s in sites], grp
        out += [(fwd, layer, SITES.index(s), e[2]) for s, e in zip(sites, grp)]
        i += len(sites)
    return out


def covered(entries, last_layer, x_path_of_last):
    """the coverage the fixture promises, over the sites whose branch reaches an output"""
    use = [e for e in entries if x_path_of_last or not (e[1] == last_layer and SITES[e[2]] != "ffn_v")]
    kinds = all(any(e[2] == s and e[3].min() == 0 for e in use) and any(e[2] == s and e[3].max() == 1 for e in use)
                for s in range(len(SITES)))
    return kinds and any(e[3].max() == 0 for e in use) and any(e[3].min() == 1 for e in use)


def pick_seed(log, base, dpr, last_layer, x_path_of_last):
    """the first seed from `base` whose replayed draws are covered()"""
    for seed in range(base, base + 4096):
        replay = [(l_, k, Tape.draw(seed, j, m.numel(), 1.0 - dpr[l_])) for j, (l_, k, m) in enumerate(log)]
        if covered(sited(replay), last_layer, x_path_of_last):
            return seed
    raise AssertionError("no seed covers the cases")


def build_reference_droppath(c, case, tape):
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
    mcfg.pop("exclude_keys", None)
    mcfg.update(case["model_args"])
    mcfg["backbone"]["type"] = "MaskClipVisionTransformer"
    ccfg["type"] = "MaskClipVisionTransformer"
    mcfg["decode_head"]["type"] = "VLGHead"
    m = ref_vlm.VLM(load_text_embedding=G.TEXT, load_mcc_text_embedding=G.MCC_TEXT, load_pl_text_embedding=G.TEXT,
                    clip_encoder=ccfg, maskclip_class_filter=None, **mcfg)
    m.disable_dropout, m.fp_rate = case["disable_dropout"], 0.5
    m.forward = types.MethodType(forward_wrapper, m)
    dpr = [x.item() for x in torch.linspace(0, case["backbone"]["drop_path_rate"], c["layers"], dtype=torch.float32)]
    for i, lyr in enumerate(m.backbone.layers):
        lyr.first_iter = False
        assert isinstance(lyr.attn.dropout_layer, torch.nn.Identity) and isinstance(lyr.ffn.dropout_layer, torch.nn.Identity)
        lyr.attn.dropout_layer = DropPathRecorder(dpr[i], i, "attn", tape)
        lyr.ffn.dropout_layer = DropPathRecorder(dpr[i], i, "ffn", tape)
    if hasattr(m.backbone, "prompt_dropout"):
        m.backbone.prompt_dropout = PromptRecorder(0.1, enabled=not case["disable_dropout"])
    return m, dpr


def pack(entries):
    bits = torch.stack([e[3] for e in entries]).numpy().astype(np.uint8)
    return np.packbits(bits.ravel()), np.array(bits.shape), np.array([e[:3] for e in entries], dtype=np.int64)


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

    out = dict(cfg=np.array(repr(dict(CASES["A"]["cfg"], name="droppath"))), iters=np.array([iters, total]))

    for name, case in CASES.items():
        c = case["cfg"]
        B, S, L = c["B"], c["S"], c["layers"]
        batch = O.synthetic_batch(B, S, 21, seed=1234 + c["seed"])
        if c.get("smooth_inputs"):
            batch = smooth_batch(batch)
        g = torch.Generator().manual_seed(c["seed"] + 100)
        fp_masks = [(torch.rand(2 * B, ch, generator=g) > 0.5).float() for ch in (c["embed"], c["embed"], 512)]
        conf_thresh = c["conf_thresh"]
        enc_keys = case["enc_keys"]

        def run(sd, f64, seeds):
            """one step of the reference, then its encoder alone -> (loss, aux, grads, step log, encoder results)"""
            to = (lambda t: t.double() if t.is_floating_point() else t) if f64 else (lambda t: t)
            keep = torch.Tensor.float
            if f64:
                torch.set_default_dtype(torch.float64)
                torch.Tensor.float = lambda self, *a, **k: self.double()
            try:
                torch.manual_seed(c["seed"])
                tape = Tape()
                ref, dpr = build_reference_droppath(c, case, tape)
                ref.load_state_dict(sd, strict=True)
                assert all(p.dtype == (torch.float64 if f64 else torch.float32) for p in ref.parameters())
                tape.reset(seeds[0])
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
                step_log = list(tape.log)
                # the encoder alone, in train mode
                for p in ref.parameters():
                    p.grad = None
                tape.reset(seeds[1])
                ref.train()
                feats, glob = ref.backbone(to(batch["img_x"]))
                feats = [f.flatten(2).transpose(1, 2) for f in feats]
                cots = seeded_cots([tuple(f.shape) for f in feats], c["seed"] + 400)
                sum((f * to(ct)).sum() for f, ct in zip(feats, cots)).backward()
                bb = dict(ref.backbone.named_parameters())
                enc = dict(feats=[f.detach() for f in feats], glob=glob.detach(), log=list(tape.log),
                           grads={k: bb[k].grad.detach().clone() for k in enc_keys})
                return loss.detach(), aux, grads, step_log, enc, dpr
            finally:
                torch.Tensor.float = keep
                torch.set_default_dtype(torch.float32)

        ref, dpr = build_reference_droppath(c, case, Tape())
        sd = seeded_state([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], c["seed"], c.get("logit_gain"))
        # a first run for the call logs, then the seeds whose draws cover the cases
        _, _, _, log0, enc0, _ = run(sd, False, (c["seed"] + 200, c["seed"] + 300))
        seeds = (pick_seed(log0, c["seed"] + 200, dpr, L - 1, False), pick_seed(enc0["log"], c["seed"] + 300, dpr, L - 1, True))
        l32, _, g32, m32, e32, _ = run(sd, False, seeds)
        loss, aux, rg, step_log, enc, dpr64 = run(sd, True, seeds)
        assert dpr64 == dpr and dpr[0] == 0.0
        assert set(g32) == set(rg)
        for a, b in ((m32, step_log), (e32["log"], enc["log"])):
            assert len(a) == len(b) and all(x[:2] == y[:2] and torch.equal(x[2], y[2]) for x, y in zip(a, b))
        step_e, enc_e = sited(step_log), sited(enc["log"])
        assert covered(step_e, L - 1, False) and covered(enc_e, L - 1, True)
        assert all(e[1] > 0 for e in step_e + enc_e) and {e[0] for e in step_e} == {0, 1} and {e[0] for e in enc_e} == {0}
        assert all(e[3].numel() == 2 * B for e in step_e) and all(e[3].numel() == B for e in enc_e)
        full = case["full"]
        assert all(k in rg for k in full)

        def rel(a, b):
            return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()

        gap = {k: rel(g32[k], rg[k]) for k in full}
        ngap = {k: abs(g32[k].double().norm().item() / rg[k].norm().item() - 1) for k in rg
                if rg[k].norm() > 0 and k != "decode_head.head.bias"}      # (that one sums to zero: its norm is rounding noise)
        print(f"[droppath {name}] seeds {seeds}; float32 run: loss {l32.item():.8f} (float64 {loss.item():.8f}); full gradients, "
              f"rel max distance from the float64 run: worst {max(gap.values()):.2e} ({max(gap, key=gap.get)}); gradient norms: "
              f"worst {max(ngap.values()):.2e} ({max(ngap, key=ngap.get)})")
        egap = {k: rel(e32["grads"][k], enc["grads"][k]) for k in enc_keys}
        print(f"[droppath {name}] encoder alone, float32 run: features "
              f"{max(rel(a, b) for a, b in zip(e32['feats'], enc['feats'])):.2e}, gradients {max(egap.values()):.2e} from the "
              f"float64 run")
        loss, aux = loss.float(), {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in aux.items()}
        rg = {k: v.float() for k, v in rg.items()}
        print(f"[droppath {name}] loss {loss.item():.8f}; {len(rg)} grads, {sum(k.startswith('backbone.') for k in rg)} backbone; "
              f"{len(step_e)} step masks, {len(enc_e)} encoder masks; rates {dpr}")
        for tag, ent in (("step", step_e), ("encoder", enc_e)):
            print(f"    {tag}: " + " ".join(f"{f}/{l_}/{SITES[s_]}:" + "".join(str(int(v)) for v in m_) for f, l_, s_, m_ in ent))
        pre = name + "/"
        spec = {k: v for k, v in case.items() if k != "cfg"}
        out[pre + "case"] = np.array(repr(spec))
        out[pre + "cfg"] = np.array(repr(dict(c, name="droppath")))
        out[pre + "dpr"] = np.array(dpr, dtype=np.float64)
        out[pre + "state_keys"] = np.array(list(sd))
        out[pre + "fp_masks"] = np.concatenate([m.numpy().ravel() for m in fp_masks]).astype(np.uint8)
        out[pre + "in_checksum"] = np.array([sum(v.double().sum().item() for v in batch.values())])
        out[pre + "loss"] = loss.detach().numpy()
        for k in ("loss_x", "loss_s1", "loss_s2", "loss_fp", "loss_mc_s1", "loss_mc_s2", "loss_mc_fp"):
            out[pre + k] = aux[k].detach().numpy()
        out[pre + "grad_names"] = np.array(sorted(rg))
        out[pre + "w_checksum"] = np.array([sum(v.double().sum().item() for v in sd.values()),
                                            sum(v.double().abs().sum().item() for v in sd.values())])
        for k in sorted(rg):
            out[pre + "gnorm/" + k] = np.array([rg[k].norm().item(), rg[k].flatten()[0].item(), rg[k].flatten()[-1].item()])
        for k in full:
            out[pre + "grad/" + k] = rg[k].numpy()
        out[pre + "dp_masks"], out[pre + "dp_masks_shape"], out[pre + "dp_masks_log"] = pack(step_e)
        out[pre + "enc_masks"], out[pre + "enc_masks_shape"], out[pre + "enc_masks_log"] = pack(enc_e)
        for j, f in enumerate(enc["feats"]):
            out[pre + f"enc/feat{j}"] = (f[0, :, ::8] if f.shape[-1] == 512 else f[0]).numpy()
        out[pre + "enc/glob"] = enc["glob"].numpy()
        for k in enc_keys:
            out[pre + "enc/grad/" + k] = enc["grads"][k].numpy()
    path = os.path.join(HERE, "semivl_droppath.npz")
    np.savez_compressed(path, **out)
    print(f"    wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)")
    assert os.path.getsize(path) <= 512 * 1024


if __name__ == "__main__":
    main()
