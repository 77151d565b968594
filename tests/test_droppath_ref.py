"""tests/droppath_ref.py proved on the CPU: its two kernel restatements and its block against torch float64 autograd of
identity + branch / keep * mask[:, None, None] (the DropPath of the reference's blocks), and its encoder against the
encoder-only arrays of tests/golden/semivl_droppath.npz (the reference's own MaskClipVisionTransformer with recorded
stochastic-depth masks, run in float64).  Tolerance 1e-12 relative to each tensor's largest entry, as in test_prompt_ref.py: the
two sides differ in the order of float64 operations only (branch * (mask / keep) against branch / keep * mask)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import droppath_ref as R
from golden_util import fixture_batch, load_fixture, seeded_state

SHAPES = [(1, 1, 6), (3, 5, 64), (2, 70, 8)]      # (B, T, E)
MASKS = {1: [[0.0], [1.0]], 2: [[1.0, 0.0], [0.0, 0.0], [1.0, 1.0]], 3: [[1.0, 0.0, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]}


def _rel(got, want):
    want = np.asarray(want)
    return np.abs(np.asarray(got) - want).max() / max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("keep", [0.75, 0.5, 1.0 - 0.20000000298023224])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_restatements_are_the_autograd_of_drop_path(shape, keep):
    B, T, E = shape
    g = torch.Generator().manual_seed(B * T + E)
    for mask in MASKS[B]:
        mask = torch.tensor(mask, dtype=torch.float64)
        branch = torch.randn(B, T, E, generator=g, dtype=torch.float64).requires_grad_(True)
        ident = torch.randn(B, T, E, generator=g, dtype=torch.float64).requires_grad_(True)
        dout = torch.randn(B, T, E, generator=g, dtype=torch.float64)
        want = ident + branch / keep * mask[:, None, None]
        (want * dout).sum().backward()
        s = mask.numpy() * (1.0 / keep)
        out, mag = R.droppath_fwd_ref(branch.detach().reshape(B * T, E).numpy(), ident.detach().reshape(B * T, E).numpy(), s, T)
        assert _rel(out, want.detach().reshape(B * T, E).numpy()) <= 1e-12
        assert (mag >= np.abs(out) * (1 - 1e-12)).all()
        db = R.droppath_bwd_ref(dout.reshape(B * T, E).numpy(), s, T)
        assert _rel(db, branch.grad.reshape(B * T, E).numpy()) <= 1e-12 if mask.any() else not db.any()
        assert torch.equal(ident.grad, dout)                # the identity path takes d out unscaled
        # rows of a dropped sample: resid's own values / zeros
        drop = np.repeat(mask.numpy() == 0, T)
        assert np.array_equal(out[drop], ident.detach().reshape(B * T, E).numpy()[drop]) and not db[drop].any()


def test_dropped_samples_do_not_read_the_branch():
    """the kernels copy resid / write zeros without reading branch / dout: a NaN there does not reach the output"""
    B, T, E = 2, 3, 4
    branch, resid = np.full((B * T, E), np.nan), np.arange(B * T * E, dtype=np.float64).reshape(B * T, E)
    branch[T:] = 1.0
    out, mag = R.droppath_fwd_ref(branch, resid, np.array([0.0, 2.0]), T)
    assert np.array_equal(out[:T], resid[:T]) and np.array_equal(out[T:], resid[T:] + 2.0) and np.isfinite(mag).all()
    db = R.droppath_bwd_ref(branch, np.array([0.0, 2.0]), T)
    assert not db[:T].any() and np.array_equal(db[T:], np.full((T, E), 2.0))


def test_scale_is_the_fp32_quotient():
    for keep in (0.9, 0.75, 1.0 - 0.20000000298023224, 1.0):
        s32 = R.scale32(keep)
        assert s32 == float(torch.tensor(1.0 / keep, dtype=torch.float32).item())
        s = R.sample_scale([0.0, 1.0], s32)
        assert s.dtype == np.float64 and s[0] == 0.0 and s[1] == s32


def _block_state(E, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = {"ln1.weight": (E,), "ln1.bias": (E,), "attn.attn.in_proj_weight": (3 * E, E), "attn.attn.in_proj_bias": (3 * E,),
              "attn.attn.out_proj.weight": (E, E), "attn.attn.out_proj.bias": (E,), "ln2.weight": (E,), "ln2.bias": (E,),
              "ffn.layers.0.0.weight": (hidden, E), "ffn.layers.0.0.bias": (hidden,), "ffn.layers.1.weight": (E, hidden),
              "ffn.layers.1.bias": (E,)}
    return {"b." + k: (torch.randn(*s, generator=g, dtype=torch.float64) * (0.3 if len(s) == 2 else 1.0)
                       + (1.0 if k.endswith("weight") and len(s) == 1 else 0.0)).requires_grad_(True) for k, s in shapes.items()}


def _plain_block(sd, x, heads, masks, keep):
    """the block in the reference's words: identity + branch / keep * mask[:, None, None] at the three sites"""
    B, n, E = x.shape
    D = E // heads

    def dp(t, site):
        return t / keep * masks[site][:, None, None]

    def ln(t, k):
        return F.layer_norm(t, (E,), sd[f"b.{k}.weight"], sd[f"b.{k}.bias"], 1e-5)

    def ffn(t):
        return F.linear(F.gelu(F.linear(t, sd["b.ffn.layers.0.0.weight"], sd["b.ffn.layers.0.0.bias"])),
                        sd["b.ffn.layers.1.weight"], sd["b.ffn.layers.1.bias"])

    wo, bo = sd["b.attn.attn.out_proj.weight"], sd["b.attn.attn.out_proj.bias"]
    qkv = F.linear(ln(x, "ln1"), sd["b.attn.attn.in_proj_weight"], sd["b.attn.attn.in_proj_bias"])
    v = F.linear(qkv[..., 2 * E:], wo, bo) + x
    v = v + dp(ffn(ln(v, "ln2")), "ffn_v")
    q, k, vh = (t.reshape(B, n, heads, D).transpose(1, 2) for t in qkv.split(E, dim=-1))
    att = torch.softmax(q @ k.transpose(-1, -2) / D ** 0.5, dim=-1) @ vh
    x = x + dp(F.linear(att.transpose(1, 2).reshape(B, n, E), wo, bo), "attn")
    return x + dp(ffn(ln(x, "ln2")), "ffn"), v


@pytest.mark.parametrize("masks", [dict(attn=[1, 0, 1], ffn=[0, 1, 1], ffn_v=[1, 1, 0]), dict(attn=[0, 0, 0], ffn=[1, 1, 1], ffn_v=[0, 1, 0])],
                         ids=["mixed", "all-dropped-and-all-kept"])
def test_block_is_the_autograd_of_the_three_sites(masks):
    """block_ref runs its three sites through the kernel restatements (forward and backward); outputs and every gradient
    against autograd of the plain formula.  Each site has its own draw; the v path's residual out_proj(v) + x has none."""
    B, n, E, heads, keep = 3, 7, 16, 2, 0.75
    masks = {k: torch.tensor(v, dtype=torch.float64) for k, v in masks.items()}
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(B, n, E, generator=g, dtype=torch.float64)
    cx, cv = torch.randn(B, n, E, generator=g, dtype=torch.float64), torch.randn(B, n, E, generator=g, dtype=torch.float64)
    res = []
    for which in ("ref", "plain"):
        sd = _block_state(E, 4 * E, 11)
        x = x0.clone().requires_grad_(True)
        if which == "ref":
            xo, v = R.block_ref(sd, "b.", x, heads, True, masks={k: m.numpy() for k, m in masks.items()}, scale=1.0 / keep)
        else:
            xo, v = _plain_block(sd, x, heads, masks, keep)
        ((xo * cx).sum() + (v * cv).sum()).backward()
        res.append((xo.detach(), v.detach(), dict(sd, x=x)))
    (xa, va, ga), (xb, vb, gb) = res
    assert _rel(xa, xb) <= 1e-12 and _rel(va, vb) <= 1e-12
    for k in gb:
        assert gb[k].grad.abs().max() > 0 and _rel(ga[k].grad, gb[k].grad) <= 1e-12, k


@pytest.fixture(scope="module")
def fx():
    return load_fixture("droppath")


@pytest.mark.parametrize("name", ["A", "B"])
def test_encoder_matches_the_reference_in_float64(fx, name):
    """encoder_ref (case B: on the merged LoRA weights, with its prompt rows) against the reference's encoder in train mode, both
    in float64 on the same seeded weights, image, cotangents and recorded masks.  The reference divides by keep = 1 - dpr[i]
    in float64: the restatement takes that quotient here, not the kernels' fp32 one."""
    z, _ = fx
    case = R.Case(z, name)
    c, spec = case.cfg, case.spec
    hip = R.build_case(case)
    sd = seeded_state([(k, tuple(v.shape)) for k, v in hip.state_dict().items()], c["seed"], c.get("logit_gain"))
    chk = np.array([sum(v.double().sum().item() for v in sd.values()), sum(v.double().abs().sum().item() for v in sd.values())])
    assert np.allclose(chk, case["w_checksum"], rtol=0, atol=1e-6)
    assert [str(k) for k in case["state_keys"]] == list(sd)       # the reference's state_dict order (and key names)
    assert hip.backbone.dpr == list(case["dpr"])
    bsd = {k[len("backbone."):]: v.double() for k, v in sd.items() if k.startswith("backbone.")}
    keys = spec["enc_keys"]
    lora = any(".lora." in k for k in bsd)
    # (adapters' gradients: by the chain rule through the merged weight, dB = s dW A^T, dA = s B^T dW)
    msd = R.merge_lora(bsd, spec["backbone"]["lora_scaling"]) if lora else bsd
    wkeys = sorted({k for k in keys if ".lora." not in k} |
                   {f"{k.split('.lora.')[0]}.attn.attn.{'out_proj.weight' if k.split('.lora.')[1][2] == 'o' else 'in_proj_weight'}"
                    for k in keys if ".lora." in k})
    img = fixture_batch(case, c)["img_x"]
    table = case.dp_masks("enc_masks")
    NP = (c["S"] // 16) ** 2
    cots = R.seeded_cots([(c["B"], NP, 512 if o == c["layers"] else c["embed"]) for o in c["out_indices"]], c["seed"] + 400)
    feats, glob, grads = R.encoder_grads(msd, img, cots, wkeys, heads=c["heads"], out_indices=c["out_indices"],
                                         dpr=hip.backbone.dpr, dp_masks=lambda i, s_: table[0, i, s_].numpy(),
                                         P=spec["backbone"].get("num_prompt_tokens") or 0, eps=hip.backbone.eps)
    E, worst, zero = c["embed"], 0.0, []
    for j, f in enumerate(feats):
        worst = max(worst, _rel((f[0, :, ::8] if f.shape[-1] == 512 else f[0]).numpy(), case[f"enc/feat{j}"]))
    worst = max(worst, _rel(glob.numpy(), case["enc/glob"]))
    for k in keys:
        want = case["enc/grad/" + k]
        if ".lora." in k:
            pre, (ab, _, t) = k.split(".lora.")[0], k.split(".lora.")[1][:3]
            r0 = dict(q=0, k=E, v=2 * E, o=0)[t]
            dW = grads[f"{pre}.attn.attn.{'out_proj.weight' if t == 'o' else 'in_proj_weight'}"][r0:r0 + E]
            s_ = spec["backbone"]["lora_scaling"]
            got = s_ * dW @ bsd[f"{pre}.lora.a_{t}.weight"].t() if ab == "b" else s_ * bsd[f"{pre}.lora.b_{t}.weight"].t() @ dW
        else:
            got = grads[k]
        if not np.abs(want).max() > 0:      # behind a site that dropped every sample: exactly zero on both sides
            assert not got.any(), k
            zero.append(k)
            continue
        worst = max(worst, _rel(got.numpy(), want))
    assert len(zero) <= 1, zero
    print(f"case {name}: worst relative distance of encoder_ref from the reference (float64) {worst:.2e}")
    assert worst < 1e-12
