"""CPU: tests/text_ref.py (the float64 restatement of CLIP's text tower the GPU tests compare against) reproduces the
reference's own float64 run stored in tests/golden/text_encoder.npz."""
import torch

import text_ref as R


def test_restatement_matches_the_reference_float64_run():
    f = R.load_fixture()
    d = f["dims"]
    assert (d["context_length"], d["vocab_size"], d["transformer_width"], d["transformer_heads"], d["transformer_layers"],
            d["embed_dim"]) == (9, 40, 128, 2, 2, 32)
    tok = f["tokens"]
    assert tok.dtype == torch.int64 and tuple(tok.shape) == (5, 9) and (tok[:, 0] == 38).all()
    lengths = (tok != 0).sum(1).tolist()
    assert lengths == [2, 3, 4, 5, 6] and all(tok[r, n - 1] == 39 for r, n in enumerate(lengths))
    raw = R.encode(f["sd"], tok, normalize=False)
    out = R.encode(f["sd"], tok)
    assert raw.dtype == torch.float64
    assert (raw - f["raw"]).abs().max().item() <= 1e-12 * max(1.0, f["raw"].abs().max().item())
    assert (out - f["out"]).abs().max().item() <= 1e-12
    assert (out.norm(dim=-1) - 1).abs().max().item() <= 1e-14


def test_concept_average_matches_the_reference_arithmetic():
    f = R.load_fixture()
    assert f["counts"] == [2, 1, 2]
    avg = R.concept_avg(f["sd"], f["tokens"], f["counts"])
    assert (avg - f["avg"]).abs().max().item() <= 1e-12
    # the order matters: the mean of unit rows, normalised, is another vector
    other = R.l2norm(R.segment_mean(f["out"], f["counts"]))
    assert (other - f["avg"]).abs().max().item() > 1e-6


def test_causal_mask_is_the_upper_triangle():
    """row t of the restated attention does not move when later keys and values change; row L - 1 does when key 0 changes"""
    g = torch.Generator().manual_seed(3)
    n, L, H = 2, 7, 2
    qkv = torch.randn(n * L, 3 * 64 * H, generator=g, dtype=torch.float64)
    base = R.causal_attention(qkv, n, L, H)
    t = 3
    alt = qkv.clone().view(n, L, 3 * 64 * H)
    alt[:, t + 1:, 64 * H:] = torch.randn(n, L - t - 1, 2 * 64 * H, generator=g, dtype=torch.float64)
    got = R.causal_attention(alt.view(n * L, -1), n, L, H).view(n, L, -1)
    assert torch.equal(got[:, :t + 1], base.view(n, L, -1)[:, :t + 1])
    assert not torch.equal(got[:, t + 1:], base.view(n, L, -1)[:, t + 1:])
    assert torch.allclose(base.view(n, L, -1)[:, 0], qkv.view(n, L, -1)[:, 0, 2 * 64 * H:], rtol=0, atol=1e-15)


def test_fixture_noise_floor_is_float32_sized():
    f = R.load_fixture()
    assert 0 < f["noise_f32"] < 1e-5
