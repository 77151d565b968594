"""CPU: training without MaskCLIP guidance -- the switch of `semivl_train_step` (the reference's own test,
`cfg['maskclip_consistency_lambda'] != 0`, semivl.py:158), the `clip_encoder: null` rows of experiment 41
(tests/golden/experiment41_cfgs.json) through build_model / the optimizer's parameter groups / checkpoint.save + load, and
`data.LabeledLoader` (supervised.py:239-244) on the stub dataset and augmenter of tests/test_data_host.py."""
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = ("mmseg.vlm-dlv3p-bn12-sk4-ft-mcvitb", "mmseg.vlm-dlv3p-bn12-sk4-ftap-mcvitb",
          "mmseg.vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb")


def _null_rows():
    rows = json.load(open(os.path.join(HERE, "golden", "experiment41_cfgs.json")))
    return {k: c for k, c in rows.items() if c["model"] in MODELS and c["clip_encoder"] is None}


# ------------------------------------------------------------------------------------------------ the switch
class _Reached(Exception):
    """the step got past its checks and reached its first launch"""


class _Stub:
    decode_head = None

    def __init__(self, enc):
        self.clip_encoder = enc


@pytest.mark.parametrize("lam,on", [(0, False), (0.0, False), ([0, 0], True), ((0.1, 0), True), (0.1, True), (None, True)])
def test_guidance_predicate_truth_table(monkeypatch, lam, on):
    """A scalar 0 / 0.0 switches the guidance off; a list or tuple ([0, 0] included), a non-zero scalar and a missing key
    (today's default [0.1, 0]) keep it on.  Guided on a model without encoder: ValueError naming both settings, raised
    before the in-place CutMix of the images (the step's first launch)."""
    import noguidance_ref as R
    from semivl_amd import train as T

    def first_launch(*a):
        raise _Reached()
    monkeypatch.setattr(T, "cutmix_img_", first_launch)
    cfg = dict(conf_thresh=0.95, mcc_loss_reduce="mean")
    if lam is not None:
        cfg["maskclip_consistency_lambda"] = lam
    assert R.guided(cfg) == on
    batch = {k: torch.zeros(1) for k in ("img_x", "mask_x", "img_w", "img_s1", "img_s2", "ignore_mask", "mix1", "mix2",
                                         "ignore_mask_other", "img_s1_other", "img_s2_other", "img_w_other")}
    with pytest.raises(_Reached):                       # with an encoder every setting passes the gate
        T.semivl_train_step(_Stub(object()), batch, 1, 10, cfg)
    if on:
        with pytest.raises(ValueError, match="maskclip_consistency_lambda.*clip_encoder"):
            T.semivl_train_step(_Stub(None), batch, 1, 10, cfg)
    else:
        with pytest.raises(_Reached):
            T.semivl_train_step(_Stub(None), batch, 1, 10, cfg)
    with pytest.raises(ValueError, match="bogus"):      # mcc_loss_reduce is validated whether or not it is used
        T.semivl_train_step(_Stub(None), batch, 1, 10, dict(cfg, mcc_loss_reduce="bogus"))


def test_rows_are_recorded_unguided():
    rows = _null_rows()
    assert len(rows) == 6 and sorted({c["model"] for c in rows.values()}) == sorted(MODELS)      # 3 models x 2 splits
    for c in rows.values():
        assert c["maskclip_consistency_lambda"] == 0 and c["mcc_loss_reduce"] == "mean" and c["clip_encoder"] is None


# ------------------------------------------------------------------------------------------------ the models
@pytest.fixture(scope="module")
def pairs():
    """model name -> (the row's own build, the same row built with the guidance encoder)"""
    from semivl_amd.model.builder import build_model
    out = {}
    for c in _null_rows().values():
        if c["model"] in out:
            continue
        torch.manual_seed(3)
        plain = build_model(dict(c, allow_random_init=True))
        torch.manual_seed(3)
        guided = build_model(dict(c, allow_random_init=True, clip_encoder="mcvit16", maskclip_consistency_lambda=[0.1, 0]))
        out[c["model"]] = (plain, guided)
    return out


def test_every_null_row_builds_without_clip_encoder_keys():
    from semivl_amd.model.builder import build_model
    for name, c in _null_rows().items():
        m = build_model(dict(c, allow_random_init=True))
        assert m.clip_encoder is None, name
        assert not any("clip_encoder" in k for k in m.state_dict()), name
        assert not any("clip_encoder" in k for k, _ in m.named_parameters()), name
        with pytest.raises(RuntimeError, match="clip_encoder"):
            m.forward_maskclip(torch.zeros(1, 3, 512, 512), 0.9)


def test_other_keys_and_order_equal_the_guided_build(pairs):
    for name, (plain, guided) in pairs.items():
        gk = [k for k in guided.state_dict() if not k.startswith("clip_encoder.")]
        assert any(k.startswith("clip_encoder.") for k in guided.state_dict())
        assert list(plain.state_dict()) == gk, name
        gp = [(k, p.requires_grad) for k, p in guided.named_parameters() if not k.startswith("clip_encoder.")]
        assert [(k, p.requires_grad) for k, p in plain.named_parameters()] == gp, name
        for k, v in plain.state_dict().items():          # same seed, same construction order up to the encoder
            assert v.shape == guided.state_dict()[k].shape, (name, k)


def test_optimizer_groups_equal_the_guided_models_minus_clip_encoder(pairs):
    """The groups `optimizer_from_cfg` -> FusedAdamW builds from the row's optimizer dict (the arena itself needs the GPU:
    tests/test_noguidance_gpu.py builds the optimizer, the reducer and a checkpoint with it)."""
    from semivl_amd.optim import _trainable, mmcv_param_groups
    for c in _null_rows().values():
        plain, guided = pairs[c["model"]]
        oc = c["optimizer"]

        def groups(m):
            named = [(n, p) for n, p in m.named_parameters() if _trainable(n, p)]
            return [(g["name"], g["lr"], g["weight_decay"]) for g in
                    mmcv_param_groups(named, oc["lr"], oc["weight_decay"], oc["paramwise_cfg"]["custom_keys"])]
        gp, gg = groups(plain), groups(guided)
        assert gp and gp == [g for g in gg if not g[0].startswith("clip_encoder.")], c["model"]
        assert not any(g[0].startswith("clip_encoder.") for g in gp)


def test_checkpoint_round_trip_both_directions(pairs, tmp_path):
    from semivl_amd.checkpoint import load_checkpoint, save_checkpoint
    for name, (plain, guided) in pairs.items():
        a, b = tmp_path / "plain.pth", tmp_path / "guided.pth"
        ck = save_checkpoint(str(a), plain, None, 3)
        assert not any("clip_encoder" in k for k in ck["model"])
        ckg = save_checkpoint(str(b), guided, None, 4)
        assert any("clip_encoder" in k for k in ckg["model"])
        keep_enc = {k: v.clone() for k, v in guided.state_dict().items() if k.startswith("clip_encoder.")}
        ps, gs = {k: v.clone() for k, v in plain.state_dict().items()}, {k: v.clone() for k, v in guided.state_dict().items()}
        # guided file -> unguided model (strict): every key of the model is filled from the file, the encoder's are dropped
        assert load_checkpoint(str(b), plain, strict=True) == 4
        for k, v in plain.state_dict().items():
            assert torch.equal(v, gs[k]), (name, k)
        # unguided file -> guided model (strict): the encoder's keys are not required and stay as they were
        assert load_checkpoint(str(a), guided, strict=True) == 3
        for k, v in guided.state_dict().items():
            assert torch.equal(v, keep_enc[k] if k.startswith("clip_encoder.") else ps[k]), (name, k)
        plain.load_state_dict(ps)
        guided.load_state_dict(gs)


# ------------------------------------------------------------------------------------------------ the loader
class _HostAug:
    """Stand-in augmenter (CPU), as in tests/test_data_host.py: the labelled sample's marker value comes back as img_x."""
    device = torch.device("cpu")

    def train_l(self, img, mask):
        return img[:1, :1, 0].float().expand(3, 2, 2).contiguous(), mask[:2, :2].long()


def test_labeled_loader():
    from semivl_amd.data import LabeledLoader, StepLoader, _PrefetchLoader, epoch_order
    assert issubclass(LabeledLoader, _PrefetchLoader) and issubclass(StepLoader, _PrefetchLoader)
    assert "__iter__" not in vars(LabeledLoader) and "__iter__" not in vars(StepLoader)     # one hand-over, shared
    lab = [(torch.full((4, 4, 3), i, dtype=torch.uint8), torch.full((4, 4), i % 5, dtype=torch.uint8), str(i)) for i in range(11)]
    seen = {}
    for world in (1, 2):
        for rank in range(world):
            ld = LabeledLoader(lab, _HostAug(), batch_size=2, epoch=3, rank=rank, world=world, workers=2)
            order = epoch_order(11, 3, rank, world)
            assert len(ld) == len(order) // 2 == (5 if world == 1 else 3)          # drop_last
            got = list(ld)
            assert len(got) == len(ld)
            ids = []
            for k, b in enumerate(got):
                assert sorted(b) == ["img_x", "mask_x"]
                assert tuple(b["img_x"].shape) == (2, 3, 2, 2) and b["img_x"].dtype == torch.float32
                assert tuple(b["mask_x"].shape) == (2, 2, 2) and b["mask_x"].dtype == torch.int64
                assert b["img_x"][:, 0, 0, 0].tolist() == [float(i) for i in order[2 * k:2 * k + 2]]
                assert b["mask_x"][:, 0, 0].tolist() == [i % 5 for i in order[2 * k:2 * k + 2]]
                ids += b["img_x"][:, 0, 0, 0].tolist()
            seen[(world, rank)] = ids
    assert len(set(seen[(1, 0)])) == len(seen[(1, 0)]) == 10                       # no id twice: no `nsample` repetition
    # two ranks: the sampler pads 11 -> 12 by wrap-around (one id shared), otherwise disjoint
    both = seen[(2, 0)] + seen[(2, 1)]
    assert len(both) == 12 and len(set(both)) == 11
