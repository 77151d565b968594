"""CPU: the prompt-token parameters of the CLIP ViT (backbone=dict(..., num_prompt_tokens=P)): the reference's state_dict keys
in the reference's order (the fixture's seeded weight stream depends on it), shapes and init (maskclip_vit.py:359-368, then
init_weights), build_model, the disable_dropout plumbing, the CLIP-file load, and which tensors an optimizer may touch."""
import copy
import math
import warnings

import pytest
import torch

import prompt_ref as R
from golden_util import build_hip, fixture_state, load_fixture

KEYS = ["deep_prompt_embeddings", "prompt_proj.weight", "prompt_proj.bias", "prompt_norm.weight", "prompt_norm.bias"]
VIT = dict(img_size=(64, 64), patch_size=16, patch_bias=False, embed_dims=64, num_layers=3, num_heads=1, out_indices=[0, 1, 3],
           pre_norm=True, final_norm=True, return_clip_embed=True, return_qkv=True, norm_cfg=dict(type="LN", eps=1e-6))


@pytest.fixture(scope="module")
def fx():
    return load_fixture("prompt")


def _vit(**kw):
    from semivl_amd.model.vit import MaskClipVisionTransformer
    return MaskClipVisionTransformer(**dict(VIT, **kw))


@pytest.mark.parametrize("name", ["A", "B"])
def test_state_dict_keys_and_order_are_the_references(fx, name):
    z, _ = fx
    case = R.Case(z, name)
    hip = R.build_case(case)
    assert list(hip.state_dict()) == [str(k) for k in case["state_keys"]]
    fixture_state(case, case.cfg, hip)       # asserts the checksum of the stream regenerated in this order
    sd = hip.state_dict()
    assert [k for k in sd if "prompt" in k] == ["backbone." + k for k in KEYS]
    L, E, P = case.cfg["layers"], case.cfg["embed"], case.spec["backbone"]["num_prompt_tokens"]
    assert [tuple(sd["backbone." + k].shape) for k in KEYS] == [(L, P, E), (E, E), (E,), (E,), (E,)]
    assert hip.clip_encoder.num_prompt_tokens is None and not any("prompt" in k for k in hip.clip_encoder.state_dict())


@pytest.mark.parametrize("name", ["A", "B"])
def test_trainable_tensors_are_the_fixtures_gradient_names_plus_prompt_norm(fx, name):
    """requires_grad follows VLM.freeze (exclude_keys=['prompt'] matches prompt_norm.* too, as in the reference); the tensors
    the encoder's backward and an optimizer handle are the reference's gradient names: prompt_norm.* is not among them"""
    from semivl_amd.optim import _trainable
    z, _ = fx
    case = R.Case(z, name)
    hip = R.build_case(case)
    names = [str(n) for n in case["grad_names"] if str(n).startswith("backbone.")]
    flagged = sorted(n for n, p in hip.named_parameters() if p.requires_grad and n.startswith("backbone."))
    assert flagged == sorted(names + ["backbone.prompt_norm.weight", "backbone.prompt_norm.bias"])
    assert sorted(n for n, p in hip.named_parameters() if _trainable(n, p) and n.startswith("backbone.")) == names
    tr = hip.backbone._trainable()
    assert sorted(n for n, p in hip.backbone.named_parameters() if any(p is q for q in tr)) == [n[len("backbone."):] for n in names]
    hip.backbone._check_grad_rules(tr)
    assert not any("prompt_norm" in n for n in names) and bool(case["prompt_norm_grad_is_none"][0])
    assert sum("prompt" in n for n in names) == 3


def test_init_follows_the_reference():
    """deep_prompt_embeddings: uniform(-val, val), val = sqrt(6 / (3 * patch^2 + E)); prompt_proj: kaiming_normal_(fan_out) in
    the constructor, then init_weights' random branch re-initialises every nn.Linear (trunc_normal_ std 0.02, bias 0) and
    every nn.LayerNorm (1, 0), prompt_proj and prompt_norm included"""
    torch.manual_seed(0)
    m = _vit(embed_dims=256, num_heads=4, num_prompt_tokens=20)
    val = math.sqrt(6.0 / (3 * 16 * 16 + 256))
    d = m.deep_prompt_embeddings
    assert tuple(d.shape) == (3, 20, 256) and d.abs().max() <= val and d.abs().max() > 0.99 * val
    assert abs(d.mean()) < 0.02 * val and abs(d.std() - val / math.sqrt(3)) < 0.02 * val       # 15360 uniform draws
    w = m.prompt_proj.weight
    assert abs(w.std() - 0.02) < 5e-4 and w.abs().max() <= 2.0       # trunc_normal_(std=.02), not kaiming's sqrt(2 / 256) = 0.088
    assert not m.prompt_proj.bias.any()
    assert bool((m.prompt_norm.weight == 1).all()) and not m.prompt_norm.bias.any() and m.prompt_norm.eps == 1e-6
    assert m.prompt_dropout.p == 0.1
    with pytest.raises(ValueError):
        _vit(num_prompt_tokens=0)


def test_no_prompts_gives_todays_keys(fx):
    _, c = fx
    base = build_hip(c)
    hip = R.build_hip_prompt(c, dict(num_prompt_tokens=None))
    assert list(hip.state_dict()) == list(base.state_dict())
    assert not any("prompt" in k for k in hip.state_dict()) and hip.backbone.num_prompt_tokens is None
    from semivl_amd.optim import _trainable
    assert all(_trainable(n, p) == (p.requires_grad and not n.startswith("clip_encoder.")) for n, p in hip.named_parameters())


def test_build_model_with_prompts_and_the_dropout_flag():
    from semivl_amd.model.builder import build_model, builtin_model_cfg
    from semivl_amd.synthetic import exp40_cfg
    cfg = exp40_cfg(2, 64, 21, "pascal")
    bb = copy.deepcopy(builtin_model_cfg("vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb"))["model"]["backbone"]
    bb.update(img_size=(64, 64), embed_dims=64, num_layers=2, num_heads=1, out_indices=[0, 2], num_prompt_tokens=4)
    head = copy.deepcopy(builtin_model_cfg("vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb"))["model"]["decode_head"]
    head.update(img_size=64, num_classes=21, skip_in_channels=(64, 64))
    for flag in (True, False):
        cfg.update(disable_dropout=flag, model_args=dict(maskclip_class_filter=None, backbone=dict(bb), decode_head=dict(head),
                                                         freeze_backbone=True, exclude_keys=["prompt"]))
        m = build_model(cfg)
        assert m.backbone.num_prompt_tokens == 4 and m.disable_dropout is flag and m.backbone.disable_dropout is flag
        assert tuple(m.backbone.deep_prompt_embeddings.shape) == (2, 4, 64)
        assert sorted(n for n, p in m.backbone.named_parameters() if p.requires_grad) == sorted(KEYS)
    assert _vit(num_prompt_tokens=2).disable_dropout is True and _vit().disable_dropout is True      # the default, as for VLM


def test_clip_file_load_keeps_the_prompt_init_and_does_not_warn(tmp_path):
    torch.manual_seed(1)
    src = _vit()
    sd = {"backbone." + k: (v[:, :, 0, 0].clone() if k == "proj.weight" else v.clone()) for k, v in src.state_dict().items()}
    path = str(tmp_path / "clip.pth")
    torch.save(dict(state_dict=sd), path)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = _vit(pretrained=path, num_prompt_tokens=3)
    assert not [x for x in w if "missing keys" in str(x.message)], [str(x.message) for x in w]
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    val = math.sqrt(6.0 / (3 * 16 * 16 + 64))
    assert 0.5 * val < m.deep_prompt_embeddings.abs().max() <= val       # the constructor's init, untouched by the load
    assert m.prompt_proj.weight.std() > 0.1                              # kaiming_normal_(fan_out): sqrt(2 / 64) = 0.18
    # a key the file really lacks still warns
    del sd["backbone.ln0.bias"]
    torch.save(dict(state_dict=sd), path)
    with pytest.warns(UserWarning, match="ln0.bias"):
        _vit(pretrained=path, num_prompt_tokens=3)
