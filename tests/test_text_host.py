"""CPU: the host side of the text-embedding path: convert_clip_text, CLIPTextEncoder's construction and dimension inference,
the `.concepts.json` sidecar of get_class_to_concept_idxs, and cfg['text_embedding_files'] in build_model."""
import json
import os

import numpy as np
import pytest
import torch

import text_ref as R
from semivl_amd.checkpoint import convert_clip_text, convert_clip_visual
from semivl_amd.model.text_encoder import CLIPTextEncoder


def clip_like_state(dtype=torch.float16, **dims):
    d = dict(context_length=9, vocab_size=40, width=128, layers=2, embed_dim=32)
    d.update(dims)
    sd = R.seeded_clip_text_state(d["context_length"], d["vocab_size"], d["width"], d["layers"], d["embed_dim"], 5, dtype=dtype)
    text_keys = set(sd)
    sd["visual.proj"] = torch.randn(16, d["embed_dim"]).to(dtype)
    sd["visual.class_embedding"] = torch.randn(16).to(dtype)
    sd["visual.transformer.resblocks.0.attn.in_proj_weight"] = torch.randn(48, 16).to(dtype)
    sd["visual.transformer.resblocks.0.ln_1.weight"] = torch.randn(16).to(dtype)
    sd["visual.positional_embedding"] = torch.randn(5, 16).to(dtype)
    sd["logit_scale"] = torch.tensor(4.6052)
    sd["input_resolution"] = torch.tensor(224)
    sd["context_length"] = torch.tensor(d["context_length"])
    sd["vocab_size"] = torch.tensor(d["vocab_size"])
    return sd, text_keys


def test_convert_clip_text_key_set_and_dtypes():
    sd, text_keys = clip_like_state()
    before = {k: v.clone() for k, v in sd.items()}
    res = convert_clip_text(sd)
    assert set(res) == {"meta", "state_dict"} and res["meta"] == {}
    out = res["state_dict"]
    assert set(out) == text_keys
    assert len(out) == 5 + 12 * 2
    for k, v in out.items():
        assert v.dtype == torch.float32 and torch.equal(v, sd[k].float()), k
        assert v.data_ptr() != sd[k].data_ptr()
    assert all(torch.equal(sd[k], before[k]) and sd[k].dtype == before[k].dtype for k in sd)     # the source is left alone
    assert not any(k.startswith("visual.") or k in ("logit_scale", "input_resolution", "context_length", "vocab_size") for k in out)
    with pytest.raises(ValueError, match="text tower"):
        convert_clip_text({k: v for k, v in sd.items() if k.startswith("visual.")})
    # the visual conversion does not see the text keys, as before
    vis = convert_clip_visual(sd, backbone=True)["state_dict"]
    assert not any("token_embedding" in k or "ln_final" in k for k in vis)


def test_from_clip_state_dict_infers_every_dimension():
    sd, text_keys = clip_like_state(context_length=11, vocab_size=50, width=192, layers=3, embed_dim=24)
    enc = CLIPTextEncoder.from_clip_state_dict(sd)
    assert (enc.context_length, enc.vocab_size, enc.width, enc.heads, enc.layers, enc.embed_dim) == (11, 50, 192, 3, 3, 24)
    own = enc.state_dict()
    assert set(own) == text_keys
    for k, v in own.items():
        assert v.dtype == torch.float32 and torch.equal(v, sd[k].float()), k     # the fp16 archive became fp32
    assert all(not p.requires_grad for p in enc.parameters())
    # the converted file's dict loads alike
    enc2 = CLIPTextEncoder.from_clip_state_dict(convert_clip_text(sd))
    assert all(torch.equal(a, b) for a, b in zip(enc.state_dict().values(), enc2.state_dict().values()))


def test_state_dict_keys_are_the_fixture_s():
    f = R.load_fixture()
    d = f["dims"]
    enc = CLIPTextEncoder(**d)
    own = enc.state_dict()
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in f["sd"].items()}
    enc.load_state_dict(f["sd"], strict=True)
    assert all(not p.requires_grad for p in enc.parameters())


def test_refusals():
    with pytest.raises(NotImplementedError, match="transformer_width"):
        CLIPTextEncoder(context_length=9, vocab_size=40, transformer_width=128, transformer_heads=4, transformer_layers=1, embed_dim=8)
    with pytest.raises(NotImplementedError, match="transformer_heads"):
        CLIPTextEncoder(context_length=9, vocab_size=40, transformer_width=128, transformer_heads=0, transformer_layers=1, embed_dim=8)
    with pytest.raises(NotImplementedError, match="context_length"):
        CLIPTextEncoder(context_length=193, vocab_size=40, transformer_width=64, transformer_heads=1, transformer_layers=1, embed_dim=8)
    with pytest.raises(NotImplementedError, match="context_length"):
        CLIPTextEncoder(context_length=0, vocab_size=40, transformer_width=64, transformer_heads=1, transformer_layers=1, embed_dim=8)
    CLIPTextEncoder(context_length=192, vocab_size=4, transformer_width=64, transformer_heads=1, transformer_layers=1, embed_dim=8)
    sd, _ = clip_like_state(width=96)                       # 96 // 64 = 1 head of dim 96
    with pytest.raises(NotImplementedError, match="transformer_width 96"):
        CLIPTextEncoder.from_clip_state_dict(sd)
    sd, _ = clip_like_state()
    with pytest.raises(ValueError, match="text_projection"):
        CLIPTextEncoder.from_clip_state_dict({k: v for k, v in sd.items() if k != "text_projection"})
    with pytest.raises(ValueError, match="resblocks"):
        CLIPTextEncoder.from_clip_state_dict({k: v for k, v in sd.items() if not k.startswith("transformer.resblocks.0.")})
    enc = CLIPTextEncoder.from_clip_state_dict(sd)
    with pytest.raises(RuntimeError, match="GPU"):            # no host path
        enc(torch.zeros(1, 9, dtype=torch.int64))


# ---- sidecar ---------------------------------------------------------------------------------------------------------------
def test_sidecar_concept_counts(tmp_path):
    from semivl_amd.model.text_embeddings import concept_offsets, get_class_to_concept_idxs
    npy = tmp_path / "mine_concept.npy"
    np.save(npy, np.zeros((6, 4), dtype=np.float32))
    with pytest.raises(ValueError):                            # no sidecar: as before
        get_class_to_concept_idxs(str(npy))
    with pytest.raises(ValueError):
        get_class_to_concept_idxs(str(tmp_path / "absent.npy"))
    (tmp_path / "mine_concept.concepts.json").write_text(json.dumps({"counts": [3, 1, 2]}))
    got = get_class_to_concept_idxs(str(npy))
    assert got == {0: [0, 1, 2], 1: [3], 2: [4, 5]}
    assert concept_offsets(got, "cpu").tolist() == [0, 3, 4, 6]
    # relative to the working directory too, as the model resolves the .npy
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert get_class_to_concept_idxs("mine_concept.npy") == got
    finally:
        os.chdir(cwd)
    # the two built-in names answer as before, sidecar or not
    voc = get_class_to_concept_idxs("configs/_base_/datasets/text_embedding/voc12_wbg_concept4_single.npy")
    assert len(voc) == 21 and len(voc[0]) == 45 and voc[20][-1] == 97
    for bad in ({"counts": [3, 0, 3]}, {"counts": []}, {"counts": "3"}, {"n": [1]}, {"counts": [1.5, 4.5]}):
        (tmp_path / "mine_concept.concepts.json").write_text(json.dumps(bad))
        with pytest.raises(ValueError, match="counts"):
            get_class_to_concept_idxs(str(npy))


# ---- cfg['text_embedding_files'] ---------------------------------------------------------------------------------------------
def _files(tmp_path):
    single, concept, other = tmp_path / "s.npy", tmp_path / "c.npy", tmp_path / "o.npy"
    np.save(single, np.zeros((3, 512), dtype=np.float32))
    np.save(concept, np.zeros((6, 512), dtype=np.float32))
    np.save(other, np.zeros((4, 512), dtype=np.float32))
    (tmp_path / "c.concepts.json").write_text(json.dumps({"counts": [3, 1, 2]}))
    return str(single), str(concept), str(other)


def test_text_embedding_files_validation(tmp_path):
    from semivl_amd.model.builder import text_embedding_files
    single, concept, other = _files(tmp_path)
    assert text_embedding_files(dict(text=single), 3) == dict(text=single, mcc=single, pl=single)
    assert text_embedding_files(dict(text=single, mcc=concept), 3) == dict(text=single, mcc=concept, pl=single)
    assert text_embedding_files(dict(text=single, mcc=concept, pl=single), 3)["pl"] == single
    with pytest.raises(ValueError, match="'txt'"):
        text_embedding_files(dict(text=single, txt=single), 3)
    with pytest.raises(ValueError, match="'mcc'"):
        text_embedding_files(dict(text=single, mcc=7), 3)
    with pytest.raises(ValueError, match="'text'"):
        text_embedding_files(dict(text=None), 3)
    with pytest.raises(ValueError, match="'text'"):
        text_embedding_files(dict(mcc=concept), 3)
    with pytest.raises(ValueError, match="dict"):
        text_embedding_files([single], 3)
    with pytest.raises(ValueError, match="'pl'"):
        text_embedding_files(dict(text=single, pl=concept), 3)
    # row counts, at build time
    with pytest.raises(ValueError, match="4 rows"):
        text_embedding_files(dict(text=single, mcc=other), 3)                  # neither nclass rows nor a sidecar
    with pytest.raises(ValueError, match="nclass = 4"):
        text_embedding_files(dict(text=other, mcc=concept), 4)                 # the sidecar counts number 3 classes
    (tmp_path / "c.concepts.json").write_text(json.dumps({"counts": [3, 1, 1]}))
    with pytest.raises(ValueError, match="6 rows"):
        text_embedding_files(dict(text=single, mcc=concept), 3)                # counts cover 5 rows of 6
    with pytest.raises(ValueError, match="no file"):
        text_embedding_files(dict(text=str(tmp_path / "absent.npy")), 3)


def test_build_model_lookup_is_unchanged_without_the_key(tmp_path):
    from semivl_amd.model.builder import build_model
    cfg = dict(model="mmseg.vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb", nclass=3, crop_size=32, dataset="custom",
               text_embedding_variant="single", mcc_text="single", pl_text="single", clip_encoder=None,
               disable_dropout=True, fp_rate=0.5, allow_random_init=True)
    with pytest.raises(KeyError):
        build_model(cfg)
    single, concept, other = _files(tmp_path)
    with pytest.raises(ValueError, match="'nope'"):
        build_model(dict(cfg, text_embedding_files=dict(text=single, nope=single)))
    with pytest.raises(ValueError, match="4 rows"):
        build_model(dict(cfg, text_embedding_files=dict(text=single, mcc=other)))
