"""`CLIPTextEncoder`: CLIP's text tower (third_party/zegclip/models/backbones/text_encoder.py:22-87, utils.py:124-181) on the
HIP kernel library, forward only.

The tower is frozen: it turns a class list into text embeddings once per dataset (tools/text_embeddings.py); nothing of it
runs inside a training step.  `state_dict` keys are the reference's, which are CLIP's own, so the text half of a CLIP archive
loads as it is (checkpoint.convert_clip_text).  Head dim 64 and a context of at most 192 tokens are what the causal attention
kernel takes (svl_causal_attn_fwd_f32); every CLIP text tower published so far is inside that.
"""
import re

import torch
import torch.nn as nn

from .. import ops
from ..checkpoint import clip_text_keys

_HEAD_DIM, _MAX_CONTEXT = 64, 192


class _Linear(nn.Module):
    """weight [out, in] + bias, as nn.Linear's keys; the product itself is ops.linear"""

    def __init__(self, fin, fout, std):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(fout, fin) * std, requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(fout), requires_grad=False)


class _LayerNorm(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(width), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(width), requires_grad=False)


class _Attention(nn.Module):
    """nn.MultiheadAttention's keys: in_proj_weight [3 W, W], in_proj_bias [3 W], out_proj.{weight, bias}"""

    def __init__(self, width, attn_std, proj_std):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.randn(3 * width, width) * attn_std, requires_grad=False)
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width), requires_grad=False)
        self.out_proj = _Linear(width, width, proj_std)


class _Mlp(nn.Module):
    def __init__(self, width, fc_std, proj_std):
        super().__init__()
        self.c_fc = _Linear(width, 4 * width, fc_std)
        self.c_proj = _Linear(4 * width, width, proj_std)


class _Block(nn.Module):
    def __init__(self, width, attn_std, proj_std, fc_std):
        super().__init__()
        self.attn = _Attention(width, attn_std, proj_std)
        self.ln_1 = _LayerNorm(width)
        self.mlp = _Mlp(width, fc_std, proj_std)
        self.ln_2 = _LayerNorm(width)


class _Transformer(nn.Module):
    def __init__(self, width, layers):
        super().__init__()
        proj_std = (width ** -0.5) * ((2 * layers) ** -0.5)      # CLIP's initialisation
        self.resblocks = nn.ModuleList(_Block(width, width ** -0.5, proj_std, (2 * width) ** -0.5) for _ in range(layers))


class _Embedding(nn.Module):
    def __init__(self, vocab, width):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(vocab, width) * 0.02, requires_grad=False)


class CLIPTextEncoder(nn.Module):
    def __init__(self, context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8,
                 transformer_layers=12, embed_dim=512):
        super().__init__()
        if transformer_heads < 1 or transformer_width != _HEAD_DIM * transformer_heads:
            raise NotImplementedError(f"CLIPTextEncoder: transformer_width {transformer_width} over transformer_heads "
                                      f"{transformer_heads} is not a head dim of {_HEAD_DIM}")
        if not 1 <= context_length <= _MAX_CONTEXT:
            raise NotImplementedError(f"CLIPTextEncoder: context_length {context_length} outside [1, {_MAX_CONTEXT}]")
        self.context_length, self.vocab_size = context_length, vocab_size
        self.width, self.heads, self.layers, self.embed_dim = transformer_width, transformer_heads, transformer_layers, embed_dim
        self.transformer = _Transformer(transformer_width, transformer_layers)
        self.token_embedding = _Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.randn(context_length, transformer_width) * 0.01, requires_grad=False)
        self.ln_final = _LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.randn(transformer_width, embed_dim) * transformer_width ** -0.5,
                                            requires_grad=False)

    @classmethod
    def from_clip_state_dict(cls, sd):
        """The encoder of a CLIP state dict (the archive's, or a converted file's `state_dict`): every dimension is read off
        the tensor shapes, heads = width // 64, layers = the number of `transformer.resblocks`; fp16 tensors become fp32."""
        if "token_embedding.weight" not in sd and isinstance(sd.get("state_dict"), dict):
            sd = sd["state_dict"]
        text = {k: sd[k] for k in clip_text_keys(sd)}
        for k in ("token_embedding.weight", "positional_embedding", "text_projection", "ln_final.weight"):
            if k not in text:
                raise ValueError(f"CLIPTextEncoder.from_clip_state_dict: no {k!r} in the state dict")
        vocab, width = text["token_embedding.weight"].shape
        blocks = {int(m.group(1)) for m in (re.match(r"transformer\.resblocks\.(\d+)\.", k) for k in text) if m}
        if blocks != set(range(len(blocks))) or not blocks:
            raise ValueError(f"CLIPTextEncoder.from_clip_state_dict: transformer.resblocks indices {sorted(blocks)} are not "
                             f"0 .. n-1")
        enc = cls(context_length=text["positional_embedding"].shape[0], vocab_size=vocab, transformer_width=width,
                  transformer_heads=width // _HEAD_DIM, transformer_layers=len(blocks),
                  embed_dim=text["text_projection"].shape[1])
        enc.load_state_dict({k: v.detach().float() for k, v in text.items()}, strict=True)
        return enc

    def forward(self, tokens):
        """tokens int64 [n, context_length] -> [n, embed_dim]: the projected feature at each row's EOT (its largest id)."""
        H, Lc = self.heads, self.context_length
        dev = self.positional_embedding.device
        if dev.type != "cuda":
            raise RuntimeError("CLIPTextEncoder: the parameters are not on the GPU (there is no host path)")
        if tokens.dim() != 2 or tokens.shape[1] != Lc:
            raise ValueError(f"CLIPTextEncoder: tokens must be [n, {Lc}], got {tuple(tokens.shape)}")
        with torch.no_grad():
            tokens = tokens.to(device=dev, dtype=torch.int64).contiguous()
            n = tokens.shape[0]
            x, eot = ops.text_embed(tokens, self.token_embedding.weight, self.positional_embedding)
            for blk in self.transformer.resblocks:
                y, _ = ops.layernorm_fwd(x, blk.ln_1.weight, blk.ln_1.bias, 1e-5)
                qkv = ops.linear(y, blk.attn.in_proj_weight, blk.attn.in_proj_bias)
                a = ops.causal_attn_fwd(qkv, n, Lc, H)
                x = ops.linear(a, blk.attn.out_proj.weight, blk.attn.out_proj.bias, resid=x)
                y, _ = ops.layernorm_fwd(x, blk.ln_2.weight, blk.ln_2.bias, 1e-5)
                h = ops.linear(y, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias)
                ops.quickgelu(h, out=h)
                x = ops.linear(h, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias, resid=x)
            # the EOT rows first: ln_final and the projection then see n rows, not n * L
            r = ops.gather_rows(x, eot, Lc)
            r, _ = ops.layernorm_fwd(r, self.ln_final.weight, self.ln_final.bias, 1e-5)
            return ops.matmul_nn(r, self.text_projection)

    def encode(self, tokens, normalize=True):
        out = self.forward(tokens)
        if normalize:
            with torch.no_grad():
                out, _ = ops.l2norm_fwd(out)
        return out
