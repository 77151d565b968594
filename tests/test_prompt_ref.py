"""tests/prompt_ref.py proved on the CPU: its two kernel restatements against torch.cat / slicing / nn.Dropout-style arithmetic
and float64 autograd, and its encoder against the encoder-only arrays of tests/golden/semivl_prompt.npz (the reference's own
MaskClipVisionTransformer with prompt tokens, run in float64)."""
import numpy as np
import pytest
import torch

import prompt_ref as R
from golden_util import fixture_batch, load_fixture, seeded_state

SHAPES = [(1, 2, 1, 6), (3, 4, 5, 64), (2, 9, 10, 770)]      # (B, T, P, E)


def _data(B, T, P, E, seed=0):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(B, T, E, generator=g, dtype=torch.float64)
    emb = torch.randn(P, E, generator=g, dtype=torch.float64)
    mask = (torch.rand(B, P, E, generator=g) < 0.9).double()
    return src, emb, mask


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_rows_fwd_is_cat_of_dropout(shape, masked):
    """expand: cat(x[:, :1], dropout(emb.expand(B)), x[:, 1:]) with dropout = x * (mask / (1 - p)) (the quotient is the fp32
    scale); in place: the same rows written into an existing matrix, every other row untouched"""
    B, T, P, E = shape
    src, emb, mask = _data(*shape)
    m = mask if masked else None
    rows = emb.expand(B, -1, -1)
    if masked:
        rows = rows * (mask * torch.tensor(R.SCALE, dtype=torch.float64))
    want = torch.cat((src[:, :1], rows, src[:, 1:]), dim=1).numpy()
    got = R.rows_fwd_ref(emb.numpy(), None if m is None else m.numpy(), R.SCALE, src=src.numpy())
    assert got.shape == (B, T + P, E) and np.array_equal(got, want)
    old = np.random.default_rng(1).standard_normal((B, T + P, E))
    got = R.rows_fwd_ref(emb.numpy(), None if m is None else m.numpy(), R.SCALE, dst=old)
    assert np.array_equal(got[:, 1:1 + P], want[:, 1:1 + P])
    assert np.array_equal(got[:, 0], old[:, 0]) and np.array_equal(got[:, 1 + P:], old[:, 1 + P:])


def test_scale_is_the_fp32_quotient():
    """nn.Dropout(0.1) multiplies by 1 / (1 - p) in the tensor's dtype: in fp32, float32(1 / 0.9)"""
    x = torch.ones(4096)
    torch.manual_seed(0)
    y = torch.nn.functional.dropout(x, 0.1, True)
    kept = y[y != 0]
    assert 0 < kept.numel() < x.numel() and bool((kept == kept[0]).all())
    assert float(kept[0]) == R.SCALE == float(np.float32(1.0 / 0.9))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_rows_bwd_is_the_autograd_of_fwd(shape, masked):
    """demb is d <dst, dx> / d emb of the forward (float64 autograd), with and without an accumulation base; zeroed / compact
    are dx with the prompt rows cleared / removed; the magnitude is the sum of the absolute terms"""
    B, T, P, E = shape
    src, emb, mask = _data(*shape)
    dx = torch.randn(B, T + P, E, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    emb = emb.clone().requires_grad_(True)
    src = src.clone().requires_grad_(True)
    rows = emb.expand(B, -1, -1)
    if masked:
        rows = rows * (mask * R.SCALE)
    (torch.cat((src[:, :1], rows, src[:, 1:]), dim=1) * dx).sum().backward()
    m = mask.numpy() if masked else None
    demb, mag, zeroed, compact = R.rows_bwd_ref(dx.numpy(), P, m, R.SCALE)
    assert np.abs(demb - emb.grad.numpy()).max() <= 4 * B * 2.0 ** -53 * max(mag.max(), 1e-300)
    assert np.array_equal(compact, src.grad.numpy())            # d / d src: dx without its prompt rows
    assert np.array_equal(zeroed[:, 1:1 + P], np.zeros((B, P, E)))
    assert np.array_equal(np.delete(zeroed, np.s_[1:1 + P], axis=1), compact)
    assert (mag >= np.abs(demb) * (1 - 1e-12)).all()
    base = np.random.default_rng(2).standard_normal((P, E))
    demb2, mag2, _, _ = R.rows_bwd_ref(dx.numpy(), P, m, R.SCALE, demb0=base)
    assert np.allclose(demb2, demb + base, rtol=0, atol=1e-14 * mag2.max()) and np.array_equal(mag2, mag + np.abs(base))


@pytest.fixture(scope="module")
def fx():
    return load_fixture("prompt")


@pytest.mark.parametrize("name", ["A", "B"])
def test_encoder_matches_the_reference_in_float64(fx, name):
    """encoder_ref against the reference's encoder, both in float64 on the same seeded weights, image, cotangents and
    dropout masks.  The two differ only in the order of float64 operations (fused attention / layer_norm calls against the
    reference's module calls), 3 blocks deep: 1e-12 relative to each tensor's largest entry is some 1e4 float64 roundings --
    far above what three blocks accumulate (measured: 1.1e-15) and six orders below the float32 run's own distance (about
    1e-6, printed by the generator).  The reference's float64 run divides the mask by 1 - p in float64, so the restatement
    takes the float64 quotient here (the fp32 one, R.SCALE, moves the gradients by 3.6e-11: LayerNorm removes a row's scale)."""
    z, _ = fx
    case = R.Case(z, name)
    c = case.cfg
    hip = R.build_case(case)
    sd = seeded_state([(k, tuple(v.shape)) for k, v in hip.state_dict().items()], c["seed"], c.get("logit_gain"))
    chk = np.array([sum(v.double().sum().item() for v in sd.values()), sum(v.double().abs().sum().item() for v in sd.values())])
    assert np.allclose(chk, case["w_checksum"], rtol=0, atol=1e-6)
    assert [str(k) for k in case["state_keys"]] == list(sd)       # the reference's state_dict order (and key names)
    bsd = {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}
    img = fixture_batch(case, c)["img_x"]
    masks = case.prompt_masks("enc_masks")
    assert (masks is None) == case.spec["disable_dropout"]
    P = case.spec["backbone"]["num_prompt_tokens"]
    NP = (c["S"] // 16) ** 2
    shapes = [(c["B"], NP, 512 if o == c["layers"] else c["embed"]) for o in c["out_indices"]]
    cots = R.seeded_cots(shapes, c["seed"] + 400)
    feats, glob, grads = R.encoder_prompt_grads(bsd, img, cots, heads=c["heads"], out_indices=c["out_indices"], P=P,
                                                masks=None if masks is None else list(masks), eps=hip.backbone.eps,
                                                scale=1.0 / (1.0 - 0.1))
    worst = 0.0
    for j, f in enumerate(feats):
        want = case[f"enc/feat{j}"]
        got = (f[0, :, ::8] if f.shape[-1] == 512 else f[0]).numpy()
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    worst = max(worst, np.abs(glob.numpy() - case["enc/glob"]).max() / np.abs(case["enc/glob"]).max())
    for k in R.PROMPT_KEYS:
        want = case["enc/grad/" + k]
        assert np.abs(want).max() > 0
        worst = max(worst, np.abs(grads[k].numpy() - want).max() / np.abs(want).max())
    print(f"case {name}: worst relative distance of encoder_ref from the reference (float64) {worst:.2e}")
    assert worst < 1e-12
    assert bool(case["prompt_norm_grad_is_none"][0])
