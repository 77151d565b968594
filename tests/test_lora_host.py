"""CPU: the LoRA parameters of the CLIP ViT (backbone=dict(..., lora_layers=[...])): the reference's state_dict keys in the
reference's order (the fixture's seeded weight stream depends on it), LoRA.reset_parameters' init, which tensors train
under the two exclude_keys recipes of tests/golden/semivl_lora.npz, what is refused, and the optimizer group."""
import math

import pytest
import torch

import lora_ref as R
from golden_util import build_hip, fixture_state, load_fixture


@pytest.fixture(scope="module")
def fx():
    return load_fixture("lora")


@pytest.mark.parametrize("name", ["A", "B"])
def test_state_dict_keys_and_order_are_the_references(fx, name):
    z, c = fx
    case = R.Case(z, name)
    hip = R.build_case(c, case)
    assert list(hip.state_dict()) == [str(k) for k in case["state_keys"]]
    fixture_state(case, c, hip)       # asserts the checksum of the stream regenerated in this order
    lo = case.spec["lora"]
    keys = [k for k in hip.state_dict() if ".lora." in k]
    want = [f"backbone.layers.{i}.lora.{ab}_{t}.weight" for i in lo["lora_layers"] for t in "qkvo" if t in lo["lora_targets"]
            for ab in "ab"]
    assert keys == want
    sd = hip.state_dict()
    E, r = c["embed"], lo["lora_r"]
    assert all(tuple(sd[k].shape) == ((r, E) if ".a_" in k else (E, r)) for k in keys)
    assert not any(".lora." in k for k in sd if k.startswith("clip_encoder."))


@pytest.mark.parametrize("name", ["A", "B"])
def test_trainable_backbone_tensors_are_the_fixtures_gradient_names(fx, name):
    z, c = fx
    case = R.Case(z, name)
    hip = R.build_case(c, case)
    got = sorted(n for n, p in hip.named_parameters() if p.requires_grad and n.startswith("backbone."))
    assert got == [str(n) for n in case["grad_names"] if str(n).startswith("backbone.")]
    if name == "A":
        assert got and all(".lora." in n for n in got)
    else:
        assert "backbone.pos_embed" in got and "backbone.layers.0.attn.attn.in_proj_weight" in got
        assert sum(".lora." in n for n in got) == 4


def test_init_is_lora_reset_parameters(fx):
    _, c = fx
    hip = R.build_hip_lora(c, dict(lora_layers=[0, 2], lora_r=4, lora_scaling=2.0, lora_targets="qkvo"))
    bound = 1.0 / math.sqrt(c["embed"])     # kaiming_uniform_(a=sqrt(5)): gain sqrt(2 / 6) * sqrt(3 / fan_in)
    n = 0
    for k, v in hip.backbone.state_dict().items():
        if ".lora.b_" in k:
            assert not v.any(), k
            n += 1
        elif ".lora.a_" in k:
            assert v.abs().max() <= bound and v.abs().max() > 0.5 * bound and abs(v.mean()) < 0.5 * bound, k
            n += 1
    assert n == 16


def test_lora_dropout_is_refused(fx):
    _, c = fx
    with pytest.raises(NotImplementedError):
        R.build_hip_lora(c, dict(lora_layers=[0], lora_dropout=0.1))


def test_no_adapters_gives_todays_keys(fx):
    _, c = fx
    base = build_hip(c)
    hip = R.build_hip_lora(c, dict(lora_layers=[], lora_r=8, lora_scaling=3.0, lora_targets="qv"))
    assert list(hip.state_dict()) == list(base.state_dict())
    assert not any("lora" in k for k in hip.state_dict())
    assert all(lyr.lora is None for lyr in hip.backbone.layers)


def test_adapters_take_the_backbone_learning_rate_group(fx):
    from semivl_amd.optim import mmcv_param_groups
    from semivl_amd.synthetic import exp40_cfg
    z, c = fx
    hip = R.build_case(c, R.Case(z, "A"))
    opt = exp40_cfg(1, 512, 21, "pascal")["optimizer"]
    groups = {g["name"]: g for g in mmcv_param_groups(hip.named_parameters(), opt["lr"], opt["weight_decay"],
                                                      opt["paramwise_cfg"]["custom_keys"])}
    mult = opt["paramwise_cfg"]["custom_keys"]["backbone"]["lr_mult"]
    for k in ("backbone.layers.0.lora.a_q.weight", "backbone.layers.2.lora.b_o.weight"):
        assert groups[k]["lr"] == opt["lr"] * mult and groups[k]["weight_decay"] == opt["weight_decay"]


def test_gradient_rule_check_knows_the_adapters(fx):
    z, c = fx
    hip = R.build_case(c, R.Case(z, "A"))
    hip.backbone._check_grad_rules([p for p in hip.backbone.parameters() if p.requires_grad])
