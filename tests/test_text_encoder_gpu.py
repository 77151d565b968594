"""GPU: semivl_amd.model.text_encoder.CLIPTextEncoder against the reference's float64 run (tests/golden/text_encoder.npz) and
against tests/text_ref.py at CLIP's own row geometry, in GEMM arithmetic modes 0 (fp32) and 6 (fp16 x 2 split)."""
import pytest
import torch

import text_ref as R

pytestmark = pytest.mark.gpu

LIMIT = 1e-3        # max abs on unit-norm rows: the project's feature limit


@pytest.fixture(params=[0, 6])
def mode(request):
    from semivl_amd import ops
    ops.set_gemm_emulation(request.param)
    try:
        yield request.param
    finally:
        ops.set_gemm_emulation(0)


@pytest.fixture(scope="module")
def fix():
    return R.load_fixture()


@pytest.fixture(scope="module")
def real_geometry():
    """width 512, 8 heads, context 77, 2 layers, vocabulary 512, embed 512; 6 sequences of 3 .. 77 tokens, one filling the context;
    the float64 restatement is computed once"""
    sd = R.seeded_clip_text_state(77, 512, 512, 2, 512, 21)
    tokens = R.seeded_tokens([3, 9, 77, 20, 64, 65], 77, 512, 22)
    return sd, tokens, R.encode(sd, tokens), R.encode(sd, tokens, normalize=False)


def build(sd, dev):
    from semivl_amd.model.text_encoder import CLIPTextEncoder
    return CLIPTextEncoder.from_clip_state_dict(sd).to(dev)


def test_fixture_dimensions(dev, mode, fix):
    from semivl_amd import ops
    from semivl_amd.model.text_embeddings import class_to_concept_idxs_from_counts, concept_offsets
    enc = build(fix["sd"], dev)
    out = enc.encode(fix["tokens"].to(dev))
    assert out.dtype == torch.float32 and tuple(out.shape) == (5, 32) and not out.requires_grad
    e_single = (out.cpu().double() - fix["out"]).abs().max().item()
    raw = enc.encode(fix["tokens"].to(dev), normalize=False)
    offs = concept_offsets(class_to_concept_idxs_from_counts(fix["counts"]), dev)
    avg, _ = ops.l2norm_fwd(ops.segment_mean(raw, offs))
    e_avg = (avg.cpu().double() - fix["avg"]).abs().max().item()
    print(f"text encoder, fixture dimensions, mode {mode}: single {e_single:.2e}, conceptavg {e_avg:.2e} from the reference's "
          f"float64 run (its own float32 run: {fix['noise_f32']:.2e})")
    assert e_single <= LIMIT and e_avg <= LIMIT
    assert torch.equal(enc(fix["tokens"].to(dev)), raw)            # forward() is the un-normalised embedding


def test_real_row_geometry(dev, mode, real_geometry):
    sd, tokens, ref, ref_raw = real_geometry
    enc = build(sd, dev)
    assert (enc.width, enc.heads, enc.context_length, enc.layers, enc.vocab_size, enc.embed_dim) == (512, 8, 77, 2, 512, 512)
    out = enc.encode(tokens.to(dev)).cpu()
    err = (out.double() - ref).abs().max().item()
    print(f"text encoder, width 512 x 77 tokens, mode {mode}: {err:.2e} from the float64 restatement")
    assert err <= LIMIT
    # the EOT rows: a row gathered one position off would be another vector altogether
    lengths = (tokens != 0).sum(1)
    assert tokens.argmax(-1).tolist() == (lengths - 1).tolist() and len(set(lengths.tolist())) == 6 and 77 in lengths.tolist()
    shifted = tokens.clone()
    for r, n in enumerate(lengths.tolist()):
        if n < 77:
            shifted[r, n - 1], shifted[r, n] = 1, 511        # the EOT one position later
    moved = (R.encode(sd, shifted) - ref).abs().max(dim=-1).values
    assert all(moved[r] > 20 * LIMIT for r, n in enumerate(lengths.tolist()) if n < 77), moved
    # tokens after the EOT do not reach its row: bit for bit
    g = torch.Generator().manual_seed(5)
    noisy = tokens.clone()
    for r, n in enumerate(lengths.tolist()):
        noisy[r, n:] = torch.randint(0, 510, (77 - n,), generator=g)
    assert noisy.argmax(-1).tolist() == tokens.argmax(-1).tolist() and not torch.equal(noisy, tokens)
    out2 = enc.encode(noisy.to(dev)).cpu()
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))
    # and one sequence alone gives the rows it gave in the batch
    alone = enc.encode(tokens[1:2].to(dev)).cpu()
    assert (alone.double() - ref[1:2]).abs().max().item() <= LIMIT


def test_structure(dev, fix):
    from semivl_amd.model.text_encoder import CLIPTextEncoder
    enc = CLIPTextEncoder(**fix["dims"]).to(dev)
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == {k: tuple(v.shape) for k, v in fix["sd"].items()}
    assert all(not p.requires_grad for p in enc.parameters()) and len(list(enc.buffers())) == 0
    enc.load_state_dict(fix["sd"], strict=True)
    tok = fix["tokens"].to(dev)
    with torch.enable_grad():
        out, nrm = enc(tok), enc.encode(tok)
    assert not out.requires_grad and out.grad_fn is None and not nrm.requires_grad and nrm.grad_fn is None
    with pytest.raises(ValueError, match="tokens"):
        enc(tok[:, :8])
    bad = tok.clone()
    bad[0, 1] = 40
    with pytest.raises(ValueError, match="40"):
        enc(bad)
