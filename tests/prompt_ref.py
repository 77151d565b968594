"""Float64 restatement of the two prompt-token kernels (svl_prompt_rows_fwd_f32, svl_prompt_rows_bwd_f32) and of the CLIP ViT
encoder with deep visual prompts (MaskClipVisionTransformer(num_prompt_tokens=P)) in plain torch, and the helpers the prompt
tests share (the product model at the fixture's dimensions, a per-case view of tests/golden/semivl_prompt.npz)."""
import ast
import copy

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24      # unit roundoff of fp32
SCALE = float(np.float32(1.0) / np.float32(0.9))     # 1 / (1 - p) for p = 0.1, rounded to fp32 once


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative bound of n successive fp32 roundings"""
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------ the two kernels
def rows_fwd_ref(emb, mask, scale, src=None, dst=None):
    """emb [P, E], mask [B, P, E] or None, and either src [B, T, E] (expand) or dst [B, T + P, E] (in place) -> the new
    dst [B, T + P, E] in float64: dst[b, 0] = src[b, 0], dst[b, 1 + j] = emb[j] * (mask[b, j] * scale), dst[b, 1 + P + t] =
    src[b, 1 + t]; in place only rows 1 .. P change."""
    emb = np.asarray(emb, dtype=np.float64)
    P, E = emb.shape
    assert (src is None) != (dst is None)
    if src is not None:
        src = np.asarray(src, dtype=np.float64)
        B, T, _ = src.shape
        out = np.empty((B, T + P, E))
        out[:, 0] = src[:, 0]
        out[:, 1 + P:] = src[:, 1:]
    else:
        out = np.array(dst, dtype=np.float64)
        B = out.shape[0]
    rows = np.broadcast_to(emb, (B, P, E))
    if mask is not None:
        rows = rows * (np.asarray(mask, dtype=np.float64) * np.float64(np.float32(scale)))
    out[:, 1:1 + P] = rows
    return out


def rows_bwd_ref(dx, P, mask, scale, demb0=None):
    """dx [B, T + P, E] -> (demb, mag, zeroed, compact) in float64: demb[j] = demb0[j] + sum_b dx[b, 1 + j] * (mask[b, j] *
    scale), mag the sum of the absolute terms (|demb0| included), zeroed = dx with rows 1 .. P set to zero, compact = dx
    without them [B, T, E]."""
    dx = np.asarray(dx, dtype=np.float64)
    g = dx[:, 1:1 + P]
    if mask is not None:
        g = g * (np.asarray(mask, dtype=np.float64) * np.float64(np.float32(scale)))
    demb, mag = g.sum(0), np.abs(g).sum(0)
    if demb0 is not None:
        demb, mag = demb + np.asarray(demb0, dtype=np.float64), mag + np.abs(np.asarray(demb0, dtype=np.float64))
    zeroed = dx.copy()
    zeroed[:, 1:1 + P] = 0.0
    compact = np.concatenate((dx[:, :1], dx[:, 1 + P:]), axis=1)
    return demb, mag, zeroed, compact


# ------------------------------------------------------------------------------------------------ the encoder
def encoder_ref(sd, img, heads, out_indices, P=0, masks=None, scale=SCALE, patch=16, eps=1e-5):
    """The encoder of semivl_amd.model.vit in plain torch, in the dtype of `sd` (a state_dict of the backbone: float64 here):
    -> (list of token features [B, hp * wp, C] in out_indices order, global embedding [B, 512]).  P prompt rows per block
    (masks: per layer a {0, 1} tensor [B, P, E] or None; dropout is `emb * (mask * scale)`).  Differentiable wherever a
    tensor of `sd` requires grad."""
    E = sd["cls_token"].shape[-1]
    L = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    D = E // heads
    B, _, H, W = img.shape
    hp, wp = -(-H // patch), -(-W // patch)
    x = F.conv2d(F.pad(img, (0, wp * patch - W, 0, hp * patch - H)), sd["patch_embed.projection.weight"], stride=patch)
    x = x.flatten(2).transpose(1, 2)
    assert sd["pos_embed"].shape[1] == 1 + hp * wp, "the restatement has no pos_embed resize"
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1) + sd["pos_embed"]

    def ln(t, pre):
        return F.layer_norm(t, (E,), sd[pre + ".weight"], sd[pre + ".bias"], eps)

    def ffn(t, pre):
        h = F.gelu(F.linear(t, sd[pre + "ffn.layers.0.0.weight"], sd[pre + "ffn.layers.0.0.bias"]))
        return F.linear(h, sd[pre + "ffn.layers.1.weight"], sd[pre + "ffn.layers.1.bias"])

    x = ln(x, "ln0")
    want_v = [i in out_indices or i == L - 1 for i in range(L)]
    feats, v = [], None
    for i in range(L):
        pre = f"layers.{i}."
        if P:
            emb = F.linear(sd["deep_prompt_embeddings"][i], sd["prompt_proj.weight"], sd["prompt_proj.bias"]).expand(B, -1, -1)
            if masks is not None and masks[i] is not None:
                emb = emb * (masks[i] * scale)
            x = torch.cat((x[:, :1], emb, x[:, 1:]), dim=1)
        wo, bo = sd[pre + "attn.attn.out_proj.weight"], sd[pre + "attn.attn.out_proj.bias"]
        qkv = F.linear(ln(x, pre + "ln1"), sd[pre + "attn.attn.in_proj_weight"], sd[pre + "attn.attn.in_proj_bias"])
        if want_v[i]:       # maskclip_vit.py:110-118,132: out_proj on the v slice, residual, FFN
            v = F.linear(qkv[..., 2 * E:], wo, bo) + x
            v = v + ffn(ln(v, pre + "ln2"), pre)
        n = x.shape[1]
        q, k, vh = (t.reshape(B, n, heads, D).transpose(1, 2) for t in qkv.split(E, dim=-1))
        att = torch.softmax(q @ k.transpose(-1, -2) / D ** 0.5, dim=-1) @ vh
        x = F.linear(att.transpose(1, 2).reshape(B, n, E), wo, bo) + x
        x = x + ffn(ln(x, pre + "ln2"), pre)
        if P:
            x = torch.cat((x[:, :1], x[:, 1 + P:]), dim=1)
            if want_v[i]:
                v = torch.cat((v[:, :1], v[:, 1 + P:]), dim=1)
        if i in out_indices:
            feats.append(v[:, 1:])
    x, v = ln(x, "ln1"), ln(v, "ln1")
    wproj = sd["proj.weight"].reshape(sd["proj.weight"].shape[0], E)
    if L in out_indices:
        e = F.linear(v[:, 1:], wproj)
        feats.append(e / e.norm(dim=-1, keepdim=True))
    g = F.linear(x[:, 0], wproj)
    g = g / g.norm(dim=-1, keepdim=True)
    return feats, g


PROMPT_KEYS = ("deep_prompt_embeddings", "prompt_proj.weight", "prompt_proj.bias")


def seeded_cots(shapes, seed):
    """one fp32 standard-normal cotangent per feature shape (shared with tests/golden/gen_golden_prompt.py)"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g, dtype=torch.float32) for s in shapes]


def encoder_prompt_grads(sd, img, cots, **kw):
    """(features, global, {prompt key: gradient of sum_j <feat_j, cots_j>}) of encoder_ref in float64"""
    sd = {k: v.detach().double().clone().requires_grad_(k in PROMPT_KEYS) for k, v in sd.items()}
    if kw.get("masks") is not None:
        kw = dict(kw, masks=[None if m_ is None else m_.double() for m_ in kw["masks"]])
    out = encoder_ref(sd, img.double(), **kw)
    sum((f * c.double()).sum() for f, c in zip(out[0], cots)).backward()
    return [f.detach() for f in out[0]], out[1].detach(), {k: sd[k].grad for k in PROMPT_KEYS}


# ------------------------------------------------------------------------------------------------ model helpers
class Case:
    """The keys of one case ('A' / 'B') of semivl_prompt.npz behind the interface golden_util's fixture_* helpers read
    (z.files, z[key]); .cfg: the case's fixture dimensions, .spec: its backbone arguments and recipe."""

    def __init__(self, z, name):
        self.z, self.pre = z, name + "/"
        self.files = [k[len(self.pre):] for k in z.files if k.startswith(self.pre)] + [k for k in z.files if "/" not in k]
        self.spec = ast.literal_eval(str(z[self.pre + "case"]))
        self.cfg = ast.literal_eval(str(z[self.pre + "cfg"]))

    def __getitem__(self, k):
        return self.z[self.pre + k] if (self.pre + k) in self.z.files else self.z[k]

    def prompt_masks(self, key="prompt_masks"):
        """the recorded prompt-dropout masks [calls, 2B or B, P, E] in call order, or None (dropout disabled)"""
        if key not in self.files:
            return None
        shape = [int(v) for v in self[key + "_shape"]]
        return torch.from_numpy(np.unpackbits(self[key])[:int(np.prod(shape))].reshape(shape).astype(np.float32))


def build_hip_prompt(c, backbone=None, **model_args):
    """The product model at the fixture's dimensions; `backbone`: kwargs merged into the backbone dict (what a model file
    under configs/_base_/models/ would carry), `model_args`: merged into the model dict (freeze_backbone, exclude_keys)."""
    from golden_util import MCC_TEXT, TEXT
    from semivl_amd.model.builder import VLM, builtin_model_cfg
    mcfg = copy.deepcopy(builtin_model_cfg("vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb"))["model"]
    ccfg = copy.deepcopy(builtin_model_cfg("mcvit16"))["backbone"]
    S = c["S"]
    for bb in (mcfg["backbone"], ccfg):
        bb.update(img_size=(S, S), embed_dims=c["embed"], num_layers=c["layers"], num_heads=c["heads"])
        bb.pop("pretrained", None)
    mcfg["backbone"]["out_indices"] = c["out_indices"]
    mcfg["backbone"].update(backbone or {})
    mcfg["decode_head"].update(img_size=S, num_classes=21, text_channels=c["text_channels"], up_channels=c["up"],
                               skip_in_channels=(c["embed"], c["embed"]), skip_channels=c["skip"],
                               num_heads=c["dec_heads"], channels=c["channels"])
    mcfg.pop("type")
    mcfg.pop("pretrained", None)
    mcfg.update(model_args)
    return VLM(load_text_embedding=TEXT, load_mcc_text_embedding=MCC_TEXT, load_pl_text_embedding=TEXT,
               clip_encoder=ccfg, maskclip_class_filter=None, **mcfg)


def build_case(case):
    m = build_hip_prompt(case.cfg, case.spec["backbone"], freeze_backbone=True, exclude_keys=case.spec["exclude_keys"])
    m.disable_dropout = m.backbone.disable_dropout = case.spec["disable_dropout"]
    return m


class MaskQueue:
    """backbone.prompt_mask_hook fed from recorded masks in call order"""

    def __init__(self, masks, dev):
        self.masks, self.i, self.dev = masks, 0, dev

    def __call__(self, layer, n):
        m_ = self.masks[self.i]
        self.i += 1
        assert m_.shape[0] == n, (m_.shape, n)
        return m_.to(self.dev)
