"""CPU: the DeepLabV3+ ablation rows of the reference's experiment 41 (`mmseg.vlm-dlv3p-bn12-sk4-{ft,ftap}-mcvitb`) build
through `build_model` from the reference's own flat experiment dicts (tests/golden/experiment41_cfgs.json, dumped by
tests/golden/gen_golden_cfgs41.py), carry the reference head's `state_dict` keys (tests/golden/dlv3p_head.npz), freeze
what `freeze(exclude_keys)` freezes and put the decode head's `head.*` tensors at lr x 10 like mmcv's paramwise_cfg; the
rows that stay unsupported keep raising."""
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = ("mmseg.vlm-dlv3p-bn12-sk4-ft-mcvitb", "mmseg.vlm-dlv3p-bn12-sk4-ftap-mcvitb")


def _exp41():
    return json.load(open(os.path.join(HERE, "golden", "experiment41_cfgs.json")))


def _row(model):
    return next(c for c in _exp41().values() if c["model"] == model)


@pytest.fixture(scope="module")
def models():
    from semivl_amd.model.builder import build_model
    return {m: build_model(dict(_row(m), allow_random_init=True)) for m in ROWS}


def test_rows_build_on_the_cpu(models):
    from semivl_amd.model.builder import build_model
    from semivl_amd.model.dlv3p_head import DLV3PHead
    for name, m in models.items():
        assert isinstance(m.decode_head, DLV3PHead)
        assert (m.num_classes, m.decode_head.image_size, m.align_corners) == (21, 512, False)
        assert m.backbone.out_indices == [4, 12] or tuple(m.backbone.out_indices) == (4, 12)
        assert m.head_res_size((512, 512)) is None           # logits at crop / 16: the fused up-sampling loss is off
        for p in m.decode_head.parameters():
            assert torch.isfinite(p).all() and p.requires_grad
    with pytest.raises(FileNotFoundError):                   # a configured-but-missing pretrained file fails loudly
        build_model(_row(ROWS[0]))


def test_state_dict_keys_are_the_references(models):
    want = sorted(str(k) for k in np.load(os.path.join(HERE, "golden", "dlv3p_head.npz"))["state_dict_keys"])
    for m in models.values():
        assert sorted(m.decode_head.state_dict().keys()) == want
    assert "aspp.b4.gap.2.num_batches_tracked" in want and "head.6.bias" in want
    # 9 conv + BN units (6 keys each: weight, BN weight / bias / running_mean / running_var / num_batches_tracked) + head.6
    assert len(want) == 9 * 6 + 2


def test_trainable_sets(models):
    ft, ftap = (models[r] for r in ROWS)
    assert all(p.requires_grad for p in ft.backbone.parameters())
    for n, p in ftap.backbone.named_parameters():            # vlm.py:80-88 with exclude_keys=['attn', 'pos_embed']
        assert p.requires_grad == (("attn" in n) or ("pos_embed" in n)), n
    assert sum(p.requires_grad for p in ftap.backbone.parameters()) == 49


def test_head_tensors_get_ten_times_the_rate(models):
    """The parameter groups `optimizer_from_cfg` -> FusedAdamW builds from the row's optimizer dict (the optimizer's arena
    itself needs the GPU: tests/test_dlv3p_gpu.py checks the built optimizer's groups)."""
    from semivl_amd.optim import _trainable, mmcv_param_groups
    cfg = _row(ROWS[1])
    oc = cfg["optimizer"]
    named = [(n, p) for n, p in models[ROWS[1]].named_parameters() if _trainable(n, p)]
    lr = {g["name"]: g["lr"] for g in mmcv_param_groups(named, oc["lr"], oc["weight_decay"], oc["paramwise_cfg"]["custom_keys"])}
    heads = [n for n in lr if n.startswith("decode_head.head.")]
    assert len(heads) == 8 and all(lr[n] == pytest.approx(oc["lr"] * 10.0) for n in heads)
    # (mmcv matches the FIRST custom key contained in the name, longest first: every 'decode_head.*' name contains 'head')
    assert all(lr[n] == pytest.approx(oc["lr"] * 10.0) for n in lr if n.startswith("decode_head."))
    assert all(lr[n] == pytest.approx(oc["lr"] * 1e-2) for n in lr if n.startswith("backbone."))


@pytest.mark.parametrize("model", ["mmseg.vlm-dlv3p-bn11-sk4-ft-tvit-in1k", "mmseg.vlm-zegclip-rd-pt-vitb", "deeplabv3plus"])
def test_unsupported_rows_still_raise(model):
    from semivl_amd.model.builder import build_model
    cfg = dict(_row(ROWS[0]), model=model, allow_random_init=True)
    with pytest.raises(ValueError):
        build_model(cfg)
