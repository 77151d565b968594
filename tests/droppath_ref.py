"""Float64 restatement of the two stochastic-depth kernels (svl_droppath_fwd_f32, svl_droppath_bwd_f32), of one block of the
CLIP ViT with drop-path at its three sites and of the encoder built from such blocks (MaskClipVisionTransformer(
drop_path_rate=r), optionally with prompt rows) in plain torch, and the helpers the drop-path tests share (a per-case view of
tests/golden/semivl_droppath.npz, the product model of a case, the mask table behind backbone.drop_path_hook)."""
import numpy as np
import torch
import torch.nn.functional as F

import prompt_ref as PR
from prompt_ref import build_hip_prompt, gamma, seeded_cots  # noqa: F401  (shared with the tests)

SITES = ("attn", "ffn", "ffn_v")


def scale32(keep):
    """float32(1 / keep): the scale the wrappers hand to the kernels"""
    return float(np.float32(1.0 / keep))


def sample_scale(mask, scale):
    """s_b of the kernels as float64 values: the fp32 product mask[b] * float32(scale)"""
    return (np.asarray(mask, dtype=np.float32) * np.float32(scale)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the two kernels
def droppath_fwd_ref(branch, resid, s, T):
    """branch, resid [B * T, E], s [B] float64 (the per-sample factor mask_b * scale) -> (out, mag) in float64: out[b * T + t]
    = resid[...] + s[b] * branch[...], mag = |resid| + |s * branch|.  Rows with s[b] == 0 are resid's, whatever branch holds."""
    branch, resid, s = (np.asarray(a, dtype=np.float64) for a in (branch, resid, s))
    B = s.shape[0]
    assert branch.shape == resid.shape and branch.shape[0] == B * T
    sr = np.repeat(s, T)[:, None]
    term = np.where(sr == 0.0, 0.0, sr * np.where(sr == 0.0, 0.0, branch))
    return resid + term, np.abs(resid) + np.abs(term)


def droppath_bwd_ref(dout, s, T):
    """dout [B * T, E], s [B] -> dbranch = s[b] * dout in float64 (rows with s[b] == 0: zeros, whatever dout holds)"""
    dout, s = np.asarray(dout, dtype=np.float64), np.asarray(s, dtype=np.float64)
    assert dout.shape[0] == s.shape[0] * T
    sr = np.repeat(s, T)[:, None]
    return np.where(sr == 0.0, 0.0, sr * np.where(sr == 0.0, 0.0, dout))


class _DropPathFn(torch.autograd.Function):
    """identity + drop_path(branch) on [B, T, E] float64 tensors, forward and backward through the two kernel restatements"""

    @staticmethod
    def forward(ctx, branch, resid, s):
        B, T, E = branch.shape
        ctx.s, ctx.shape = s, (B, T, E)
        out, _ = droppath_fwd_ref(branch.detach().reshape(B * T, E).numpy(), resid.detach().reshape(B * T, E).numpy(), s, T)
        return torch.from_numpy(out).reshape(B, T, E)

    @staticmethod
    def backward(ctx, dout):
        B, T, E = ctx.shape
        db = droppath_bwd_ref(dout.reshape(B * T, E).numpy(), ctx.s, T)
        return torch.from_numpy(db).reshape(B, T, E), dout, None     # (the identity path takes dout as it is)


def drop_path_add(branch, resid, mask, scale):
    """resid + (mask_b * scale) * branch ([B, T, E], float64, differentiable); mask None: the plain sum"""
    if mask is None:
        return resid + branch
    return _DropPathFn.apply(branch, resid, np.asarray(mask, dtype=np.float64) * float(scale))


# ------------------------------------------------------------------------------------------------ one block, the encoder
def block_ref(sd, pre, x, heads, want_v, skip_x=False, masks=None, scale=1.0, eps=1e-5):
    """One TransformerEncoderLayer (maskclip_vit.py:110-144) on x [B, n, E] in the dtype of `sd` -> (x_out or None, v or None).
    masks: {site: mask [B] or None} over SITES, scale = 1 / keep:
        attn   x2    = x  + dp(out_proj(attention(ln1 x)))
        ffn    x_out = x2 + dp(FFN(ln2 x2))
        ffn_v  v     = vo + dp(FFN(ln2 vo)),  vo = out_proj(v slice of in_proj(ln1 x)) + x   (no drop-path on vo)"""
    masks = masks or {}
    B, n, E = x.shape
    D = E // heads

    def ln(t, name):
        return F.layer_norm(t, (E,), sd[pre + name + ".weight"], sd[pre + name + ".bias"], eps)

    def ffn(t):
        h = F.gelu(F.linear(t, sd[pre + "ffn.layers.0.0.weight"], sd[pre + "ffn.layers.0.0.bias"]))
        return F.linear(h, sd[pre + "ffn.layers.1.weight"], sd[pre + "ffn.layers.1.bias"])

    wo, bo = sd[pre + "attn.attn.out_proj.weight"], sd[pre + "attn.attn.out_proj.bias"]
    qkv = F.linear(ln(x, "ln1"), sd[pre + "attn.attn.in_proj_weight"], sd[pre + "attn.attn.in_proj_bias"])
    v = xo = None
    if want_v:
        vo = F.linear(qkv[..., 2 * E:], wo, bo) + x
        v = drop_path_add(ffn(ln(vo, "ln2")), vo, masks.get("ffn_v"), scale)
    if not skip_x:
        q, k, vh = (t.reshape(B, n, heads, D).transpose(1, 2) for t in qkv.split(E, dim=-1))
        att = torch.softmax(q @ k.transpose(-1, -2) / D ** 0.5, dim=-1) @ vh
        x2 = drop_path_add(F.linear(att.transpose(1, 2).reshape(B, n, E), wo, bo), x, masks.get("attn"), scale)
        xo = drop_path_add(ffn(ln(x2, "ln2")), x2, masks.get("ffn"), scale)
    return xo, v


def merge_lora(sd, scaling):
    """state_dict of a backbone with adapters -> the same without them, W + s * B @ A merged into the projections"""
    out = {k: v.clone() for k, v in sd.items() if ".lora." not in k}
    E = sd["cls_token"].shape[-1]
    for k in sd:
        if ".lora.b_" in k:
            pre, t = k.split(".lora.b_")[0], k.split(".lora.b_")[1][0]
            key, r0 = dict(q=("in_proj_weight", 0), k=("in_proj_weight", E), v=("in_proj_weight", 2 * E),
                           o=("out_proj.weight", 0))[t]
            out[f"{pre}.attn.attn.{key}"][r0:r0 + E] += scaling * sd[k] @ sd[f"{pre}.lora.a_{t}.weight"]
    return out


def encoder_ref(sd, img, heads, out_indices, dpr, dp_masks=None, dp_scale=None, P=0, pmasks=None, pscale=PR.SCALE, patch=16,
                eps=1e-5):
    """prompt_ref.encoder_ref with block_ref as its block: -> (token features in out_indices order, global embedding).
    dpr: the per-block rates; dp_masks(layer, site) -> mask [B] or None (None everywhere: eval mode); dp_scale(layer) -> the
    branch scale of a block (default 1 / (1 - dpr[layer]) in float64)."""
    E = sd["cls_token"].shape[-1]
    L = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    B, _, H, W = img.shape
    hp, wp = -(-H // patch), -(-W // patch)
    x = F.conv2d(F.pad(img, (0, wp * patch - W, 0, hp * patch - H)), sd["patch_embed.projection.weight"], stride=patch)
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1) + sd["pos_embed"]
    x = F.layer_norm(x, (E,), sd["ln0.weight"], sd["ln0.bias"], eps)
    want_v = [i in out_indices or i == L - 1 for i in range(L)]
    feats, v = [], None
    for i in range(L):
        if P:
            emb = F.linear(sd["deep_prompt_embeddings"][i], sd["prompt_proj.weight"], sd["prompt_proj.bias"]).expand(B, -1, -1)
            if pmasks is not None and pmasks[i] is not None:
                emb = emb * (pmasks[i] * pscale)
            x = torch.cat((x[:, :1], emb, x[:, 1:]), dim=1)
        masks = {} if dp_masks is None or dpr[i] == 0 else {s_: dp_masks(i, s_) for s_ in SITES if s_ != "ffn_v" or want_v[i]}
        sc = 1.0 if dpr[i] == 0 else (dp_scale(i) if dp_scale is not None else 1.0 / (1.0 - dpr[i]))
        x, vi = block_ref(sd, f"layers.{i}.", x, heads, want_v[i], masks=masks, scale=sc, eps=eps)
        if P:
            x = torch.cat((x[:, :1], x[:, 1 + P:]), dim=1)
            if want_v[i]:
                vi = torch.cat((vi[:, :1], vi[:, 1 + P:]), dim=1)
        if want_v[i]:
            v = vi
        if i in out_indices:
            feats.append(v[:, 1:])
    x = F.layer_norm(x, (E,), sd["ln1.weight"], sd["ln1.bias"], eps)
    v = F.layer_norm(v, (E,), sd["ln1.weight"], sd["ln1.bias"], eps)
    wproj = sd["proj.weight"].reshape(sd["proj.weight"].shape[0], E)
    if L in out_indices:
        e = F.linear(v[:, 1:], wproj)
        feats.append(e / e.norm(dim=-1, keepdim=True))
    g = F.linear(x[:, 0], wproj)
    return feats, g / g.norm(dim=-1, keepdim=True)


def encoder_grads(sd, img, cots, keys, **kw):
    """(features, global, {key: gradient of sum_j <feat_j, cots_j>}) of encoder_ref in float64"""
    sd = {k: v.detach().double().clone().requires_grad_(k in keys) for k, v in sd.items()}
    feats, glob = encoder_ref(sd, img.double(), **kw)
    sum((f * c.double()).sum() for f, c in zip(feats, cots)).backward()
    return [f.detach() for f in feats], glob.detach(), {k: sd[k].grad for k in keys}


# ------------------------------------------------------------------------------------------------ fixture and model helpers
class Case(PR.Case):
    """One case ('A' / 'B') of semivl_droppath.npz.  The recorded stochastic-depth masks: `<key>` bit-packed [calls, n] next to
    `<key>_log` [calls, 3] = (train-mode forward, layer, index into SITES) in the reference's call order."""

    def dp_masks(self, key):
        """{(forward, layer, site): fp32 mask [n]}"""
        log = self[key + "_log"]
        calls, n = [int(v) for v in self[key + "_shape"]]
        bits = np.unpackbits(self[key])[:calls * n].reshape(calls, n).astype(np.float32)
        assert len(log) == calls
        return {(int(f), int(l_), SITES[int(s_)]): torch.from_numpy(bits[j].copy()) for j, (f, l_, s_) in enumerate(log)}


def build_case(case):
    m = build_hip_prompt(case.cfg, case.spec["backbone"], **case.spec["model_args"])
    m.disable_dropout = m.backbone.disable_dropout = case.spec["disable_dropout"]
    return m


class MaskTable:
    """backbone.drop_path_hook fed from recorded masks: the k-th request for (layer, site) is train-mode forward k's.
    .used: the requests served, in order."""

    def __init__(self, table, dev):
        self.table, self.dev, self.count, self.used = table, dev, {}, []

    def __call__(self, layer, site, n):
        assert site in SITES
        k = self.count.get((layer, site), 0)
        self.count[layer, site] = k + 1
        m_ = self.table[k, layer, site]
        assert m_.shape == (n,), (layer, site, m_.shape, n)
        self.used.append((k, layer, site))
        return m_.to(self.dev)
