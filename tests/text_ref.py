"""Float64 restatement of CLIP's text tower in plain torch (third_party/zegclip/models/backbones/text_encoder.py:79-87,
utils.py:124-170), the yardstick of the text kernels and of semivl_amd.model.text_encoder.  tests/test_text_ref.py holds it
to the reference's own float64 run (tests/golden/text_encoder.npz).  Everything runs on the host; inputs of any float type are
taken to float64 first."""
import math

import torch


def _d(t):
    return t.detach().cpu().double()


def embed(tokens, table, pos):
    """tokens int64 [n, L] -> x [n, L, W] = table[tok] + pos, eot [n] = first maximum of each row"""
    tokens = tokens.cpu()
    return _d(table)[tokens] + _d(pos)[None], tokens.argmax(dim=-1)


def layernorm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * _d(w) + _d(b)


def quickgelu(x):
    return x * torch.sigmoid(1.702 * x)


def causal_attention(qkv, n, L, H):
    """qkv [n * L, 3 W] (q | k | v), W = 64 H -> [n * L, W]; query t sees keys 0 .. t, scale 64^-0.5"""
    qkv = _d(qkv)
    W = 64 * H
    q, k, v = (qkv[:, i * W:(i + 1) * W].reshape(n, L, H, 64).permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(64.0)
    s = s + torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)
    return (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(n * L, W)


def block(x, sd, pre, n, L, H):
    """one ResidualAttentionBlock on x [n * L, W]"""
    y = layernorm(x, sd[pre + "ln_1.weight"], sd[pre + "ln_1.bias"])
    qkv = y @ _d(sd[pre + "attn.in_proj_weight"]).t() + _d(sd[pre + "attn.in_proj_bias"])
    a = causal_attention(qkv, n, L, H)
    x = x + a @ _d(sd[pre + "attn.out_proj.weight"]).t() + _d(sd[pre + "attn.out_proj.bias"])
    y = layernorm(x, sd[pre + "ln_2.weight"], sd[pre + "ln_2.bias"])
    h = quickgelu(y @ _d(sd[pre + "mlp.c_fc.weight"]).t() + _d(sd[pre + "mlp.c_fc.bias"]))
    return x + h @ _d(sd[pre + "mlp.c_proj.weight"]).t() + _d(sd[pre + "mlp.c_proj.bias"])


def num_layers(sd):
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.resblocks."))


def encode(sd, tokens, normalize=True):
    """state dict with CLIP's keys, tokens int64 [n, L] -> float64 [n, embed]"""
    x, eot = embed(tokens, sd["token_embedding.weight"], sd["positional_embedding"])
    n, L, W = x.shape
    H = W // 64
    x = x.reshape(n * L, W)
    for i in range(num_layers(sd)):
        x = block(x, sd, f"transformer.resblocks.{i}.", n, L, H)
    r = x.reshape(n, L, W)[torch.arange(n), eot]
    out = layernorm(r, sd["ln_final.weight"], sd["ln_final.bias"]) @ _d(sd["text_projection"])
    return l2norm(out) if normalize else out


def l2norm(x):
    return x / x.norm(dim=-1, keepdim=True)


def segment_mean(x, counts):
    """x [m, E], counts per class -> [N, E]: the rows of each class summed in ascending order, divided by the count"""
    x = _d(x)
    out, o = [], 0
    for c in counts:
        s = x[o]
        for r in range(o + 1, o + c):
            s = s + x[r]
        out.append(s / c)
        o += c
    assert o == x.shape[0]
    return torch.stack(out)


def concept_avg(sd, tokens, counts):
    """single_template_concept_avg (model/text_embeddings.py:164-186): mean of the un-normalised embeddings, then the norm"""
    return l2norm(segment_mean(encode(sd, tokens, normalize=False), counts))


def seeded_clip_text_state(context_length, vocab_size, width, layers, embed_dim, seed, dtype=torch.float32):
    """A CLIP text state dict with CLIP's key names and lively values (LayerNorm gains around 1, non-zero biases)."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0, mean=0.0):
        return (torch.randn(*shape, generator=g) * std + mean).to(dtype)

    sd = {"positional_embedding": rn(context_length, width, std=0.1),
          "text_projection": rn(width, embed_dim, std=width ** -0.5),
          "token_embedding.weight": rn(vocab_size, width, std=0.5),
          "ln_final.weight": rn(width, std=0.1, mean=1.0), "ln_final.bias": rn(width, std=0.1)}
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        sd[p + "attn.in_proj_weight"] = rn(3 * width, width, std=2.0 * width ** -0.5)
        sd[p + "attn.in_proj_bias"] = rn(3 * width, std=0.1)
        sd[p + "attn.out_proj.weight"] = rn(width, width, std=width ** -0.5)
        sd[p + "attn.out_proj.bias"] = rn(width, std=0.1)
        sd[p + "ln_1.weight"] = rn(width, std=0.1, mean=1.0)
        sd[p + "ln_1.bias"] = rn(width, std=0.1)
        sd[p + "mlp.c_fc.weight"] = rn(4 * width, width, std=width ** -0.5)
        sd[p + "mlp.c_fc.bias"] = rn(4 * width, std=0.1)
        sd[p + "mlp.c_proj.weight"] = rn(width, 4 * width, std=(4 * width) ** -0.5)
        sd[p + "mlp.c_proj.bias"] = rn(width, std=0.1)
        sd[p + "ln_2.weight"] = rn(width, std=0.1, mean=1.0)
        sd[p + "ln_2.bias"] = rn(width, std=0.1)
    return sd


def seeded_tokens(lengths, context_length, vocab_size, seed):
    """int64 [n, context_length]: SOT = vocab - 2, `length - 2` ids below it, EOT = vocab - 1 (the row maximum), zero padding"""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(len(lengths), context_length, dtype=torch.int64)
    for r, n in enumerate(lengths):
        assert 2 <= n <= context_length
        out[r, 0] = vocab_size - 2
        out[r, 1:n - 1] = torch.randint(1, vocab_size - 2, (n - 2,), generator=g)
        out[r, n - 1] = vocab_size - 1
    return out


def load_fixture():
    """tests/golden/text_encoder.npz (gen_golden_text.py) -> dict(dims, sd (fp32 tensors under CLIP's keys), tokens, raw, out,
    counts, avg, noise_f32)"""
    import ast
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_encoder.npz"))
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w/")}
    return dict(dims=ast.literal_eval(str(z["dims"])), sd=sd, tokens=torch.from_numpy(z["tokens"]), raw=torch.from_numpy(z["raw"]),
                out=torch.from_numpy(z["out"]), counts=[int(c) for c in z["counts"]], avg=torch.from_numpy(z["avg"]),
                noise_f32=float(z["noise_f32"]))
