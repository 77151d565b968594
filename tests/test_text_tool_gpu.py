"""GPU: the path a user with their own class list walks: convert_clip_weights --text on a (synthetic) CLIP archive, the
text_embeddings tool in its three variants, then build_model with cfg['text_embedding_files'], one guided training step and
forward_maskclip aggregating concepts through the sidecar."""
import json

import numpy as np
import pytest
import torch

import text_ref as R

pytestmark = pytest.mark.gpu

LIMIT = 1e-3
MERGES = [("t", "h"), ("th", "e</w>"), ("h", "e</w>"), ("c", "a"), ("ca", "t</w>"), ("d", "o"), ("do", "g</w>"), ("a", "b"),
          ("ab", "c</w>"), ("p", "h"), ("o", "t"), ("ph", "ot"), ("o", "f</w>"), ("i", "n"), ("in", "g</w>"), ("s", "k"),
          ("sk", "y</w>"), ("e", "a"), ("ea", "r</w>"), ("b", "ea")]
CLASSES = [["the", "he", "photo"], ["cat"], ["dog", "abc"]]
TEMPLATE = "a {}"


@pytest.fixture(scope="module")
def made(tmp_path_factory, dev):
    """the archive, the merges file, the converted files and the three .npy files, made once through the tools' main()"""
    from semivl_amd.tools import convert_clip_weights, text_embeddings
    d = tmp_path_factory.mktemp("texttool")
    vocab = 512 + len(MERGES) + 2
    sd = R.seeded_clip_text_state(9, vocab, 128, 2, 512, 31, dtype=torch.float16)
    text_keys = set(sd)
    sd["visual.proj"] = torch.randn(16, 512).half()
    sd["visual.class_embedding"] = torch.randn(16).half()
    sd["visual.ln_pre.weight"] = torch.randn(16).half()
    sd["logit_scale"] = torch.tensor(4.6052)
    torch.save(sd, d / "clip.pt")
    (d / "merges.txt").write_text("#version: synthetic\n" + "\n".join(" ".join(m) for m in MERGES) + "\n", encoding="utf-8")
    (d / "classes.json").write_text(json.dumps(CLASSES))
    convert_clip_weights.main(["--src", str(d / "clip.pt"), "--backbone", "--text", "--out-dir", str(d / "pretrained")])
    conv = d / "pretrained" / "clip_ViT16_text_encoder.pth"
    for variant, clip in (("single", conv), ("concept", d / "clip.pt"), ("conceptavg", conv)):
        text_embeddings.main(["--clip", str(clip), "--bpe", str(d / "merges.txt"), "--classes", str(d / "classes.json"),
                              "--variant", variant, "--out", str(d / f"mine_{variant}.npy"), "--template", TEMPLATE])
    return d, sd, text_keys


def test_converted_file_and_embeddings(made):
    from semivl_amd.tokenizer import SimpleTokenizer
    d, sd, text_keys = made
    conv = torch.load(d / "pretrained" / "clip_ViT16_text_encoder.pth", map_location="cpu")
    assert set(conv) == {"meta", "state_dict"} and set(conv["state_dict"]) == text_keys
    assert all(v.dtype == torch.float32 and torch.equal(v, sd[k].float()) for k, v in conv["state_dict"].items())
    assert (d / "pretrained" / "clip2mmseg_ViT16_clip_backbone.pth").exists()
    tok = SimpleTokenizer(str(d / "merges.txt"))
    text = {k: sd[k] for k in text_keys}
    names = [c[0] for c in CLASSES]
    concepts = [s for c in CLASSES for s in c]
    counts = [len(c) for c in CLASSES]
    t_single = tok.tokenize([TEMPLATE.format(s) for s in names], context_length=9)
    t_concept = tok.tokenize([TEMPLATE.format(s) for s in concepts], context_length=9)
    assert t_single[1].tolist() == [tok.sot_id, tok.encoder["a</w>"], tok.encoder["cat</w>"], tok.eot_id, 0, 0, 0, 0, 0]
    want = dict(single=R.encode(text, t_single), concept=R.encode(text, t_concept),
                conceptavg=R.concept_avg(text, t_concept, counts))
    for variant, ref in want.items():
        got = np.load(d / f"mine_{variant}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(ref.shape) and got.shape[1] == 512
        err = np.abs(got.astype(np.float64) - ref.numpy()).max()
        print(f"text_embeddings --variant {variant}: {err:.2e} from the float64 restatement")
        assert err <= LIMIT
        assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() <= 1e-6
        side = d / f"mine_{variant}.concepts.json"
        assert side.exists() == (variant == "concept")
    assert json.loads((d / "mine_concept.concepts.json").read_text()) == {"counts": counts}
    # the mean comes before the norm.  The other order is another vector, but at these dimensions only a few 1e-4 away (the raw
    # rows have similar norms), which LIMIT cannot tell apart: the file must lie ten times nearer to the right order than the
    # two orders lie from each other (float32 arithmetic leaves it some 1e-7 away)
    other = R.l2norm(R.segment_mean(want["concept"], counts))
    gap = (other - want["conceptavg"]).abs().max().item()
    got = np.load(d / "mine_conceptavg.npy").astype(np.float64)
    assert gap > 1e-4 and np.abs(got - want["conceptavg"].numpy()).max() <= 0.1 * gap


def test_build_model_and_train_on_the_new_files(made, dev):
    import copy
    from golden_util import load_fixture
    from oracle import semivl_oracle as O
    from semivl_amd.model.builder import build_model, builtin_model_cfg
    from semivl_amd.model.text_embeddings import get_class_to_concept_idxs
    from semivl_amd.train import semivl_train_step
    d, _, _ = made
    _, c = load_fixture("tiny")
    S = c["S"]
    mcfg = copy.deepcopy(builtin_model_cfg("vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb"))["model"]
    ccfg = copy.deepcopy(builtin_model_cfg("mcvit16"))["backbone"]
    for bb in (mcfg["backbone"], ccfg):
        bb.update(img_size=(S, S), embed_dims=c["embed"], num_layers=c["layers"], num_heads=c["heads"])
        bb.pop("pretrained", None)
    mcfg["backbone"]["out_indices"] = c["out_indices"]
    mcfg["decode_head"].update(img_size=S, num_classes=3, text_channels=c["text_channels"], up_channels=c["up"],
                               skip_in_channels=(c["embed"], c["embed"]), skip_channels=c["skip"], num_heads=c["dec_heads"],
                               channels=c["channels"])
    files = dict(text=str(d / "mine_single.npy"), mcc=str(d / "mine_concept.npy"))
    cfg = dict(model="mmseg.vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb", nclass=3, crop_size=S, dataset="custom",
               text_embedding_files=files, clip_encoder="mcvit16", disable_dropout=True, fp_rate=0.5, allow_random_init=True,
               model_args=dict(backbone=mcfg["backbone"], decode_head=mcfg["decode_head"], clip_encoder=ccfg, pretrained=None))
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    assert model.num_classes == 3 and model.load_text_embedding == files["text"] and model.load_mcc_text_embedding == files["mcc"]
    assert tuple(model.loaded_mcc_text_feat.shape) == (6, 512) and tuple(model.text_feat(dev).shape) == (3, 512)
    assert get_class_to_concept_idxs(files["mcc"]) == {0: [0, 1, 2], 1: [3], 2: [4, 5]}
    batch = {k: v.to(dev) for k, v in O.synthetic_batch(c["B"], S, 3, seed=7).items()}
    labels = model.forward_maskclip(batch["img_w"], 0.0)            # 6 concept maps -> 3 classes through the sidecar
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (c["B"], S, S)
    assert set(labels.unique().tolist()) <= {0, 1, 2, 255}
    step_cfg = dict(conf_thresh=0.05, conf_mode="pixelwise", mcc_conf_thresh=0.0, mcc_loss_reduce="mean_all",
                    maskclip_consistency_lambda=[0.1, 0])
    losses = semivl_train_step(model, batch, 1, 10, step_cfg)
    vals = losses.detach().cpu().tolist()
    assert len(vals) == 8 and all(np.isfinite(v) for v in vals) and vals[0] > 0, vals
    # without the key the lookup is the closed one, as before
    with pytest.raises(KeyError):
        build_model({k: v for k, v in cfg.items() if k != "text_embedding_files"})
