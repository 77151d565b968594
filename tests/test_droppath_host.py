"""CPU: the stochastic-depth option of the CLIP ViT (backbone=dict(..., drop_path_rate=r)): the per-block schedule, what the
constructor accepts and still refuses, the unchanged state_dict, which sites ask backbone.drop_path_hook for a mask, build_model
and the fixture's trainable tensors."""
import pytest
import torch

import droppath_ref as R
from golden_util import fixture_state, load_fixture

VIT = dict(img_size=(64, 64), patch_size=16, patch_bias=False, embed_dims=64, num_layers=3, num_heads=1, out_indices=[0, 1, 3],
           pre_norm=True, final_norm=True, return_clip_embed=True, return_qkv=True, norm_cfg=dict(type="LN", eps=1e-6))


def _vit(**kw):
    from semivl_amd.model.vit import MaskClipVisionTransformer
    return MaskClipVisionTransformer(**dict(VIT, **kw))


@pytest.mark.parametrize("rate, layers", [(0.1, 12), (0.5, 3), (0.4, 3), (0.3, 1), (0.0, 4), (0, 2)])
def test_schedule_is_the_references_linspace(rate, layers):
    """maskclip_vit.py:299-301; block 0 and a one-layer model have rate 0"""
    bb = _vit(drop_path_rate=rate, num_layers=layers, out_indices=[layers])
    assert bb.dpr == [x.item() for x in torch.linspace(0, rate, layers)] and len(bb.dpr) == layers
    assert bb.dpr[0] == 0.0 and all(isinstance(p, float) for p in bb.dpr)
    if layers > 1 and rate:
        assert bb.dpr[-1] == torch.tensor(rate, dtype=torch.float32).item() and all(a < b for a, b in zip(bb.dpr, bb.dpr[1:]))
    assert _vit().dpr == [0.0] * 3 and _vit().drop_path_hook is None


def test_constructor_accepts_drop_path_rate_and_still_refuses_the_others():
    from semivl_amd.model.vit import DROP_PATH_SITES
    assert DROP_PATH_SITES == ("attn", "ffn", "ffn_v") == R.SITES
    _vit(drop_path_rate=0.1)
    for kw, off in ((dict(drop_rate=0.1), "'drop_rate': 0.1"), (dict(attn_drop_rate=0.1), "'attn_drop_rate': 0.1"),
                    (dict(drop_path_rate=0.1, drop_rate=0.1), "'drop_rate': 0.1"),
                    (dict(lora_layers=[1], lora_dropout=0.1), "'lora_dropout': 0.1")):
        with pytest.raises(NotImplementedError) as e:
            _vit(**kw)
        assert off in str(e.value) and "'drop_path_rate'" not in str(e.value)      # the offending option, by name and value
        assert all(n in str(e.value) for n in ("drop_rate, ", "attn_drop_rate", "lora_dropout"))    # and what stays refused
    for bad in (1.0, -0.1, 1.5, "0.1", None, True):
        with pytest.raises(ValueError):
            _vit(drop_path_rate=bad)


def test_state_dict_is_unchanged_by_the_option():
    torch.manual_seed(0)
    a = _vit()
    torch.manual_seed(0)
    b = _vit(drop_path_rate=0.3)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)      # same keys, same order, same init stream
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    b.load_state_dict(sa, strict=True)


def test_hook_is_asked_for_the_live_sites_by_name():
    """train mode, rate > 0, and only the branches the forward runs: the v path's FFN first (the reference's call order), the
    last block's x path only when it is computed; the hook's mask is taken as it is, one value per sample"""
    from semivl_amd.model.vit import _drop_path_masks
    bb = _vit(drop_path_rate=0.5, out_indices=[1, 3])
    asked = []

    def hook(layer, site, B):
        asked.append((layer, site, B))
        return torch.arange(B, dtype=torch.float32)

    bb.drop_path_hook = hook
    dev = torch.device("cpu")
    bb.train()
    assert _drop_path_masks(bb, 0, 4, False, False, dev) is None and not asked          # rate 0: the block as without the option
    dp = _drop_path_masks(bb, 1, 4, True, False, dev)
    assert asked == [(1, "ffn_v", 4), (1, "attn", 4), (1, "ffn", 4)]
    assert sorted(dp) == ["attn", "ffn", "ffn_v", "keep"] and dp["keep"] == 0.75 and torch.equal(dp["ffn"], torch.arange(4.))
    del asked[:]
    assert sorted(_drop_path_masks(bb, 2, 2, True, True, dev)) == ["ffn_v", "keep"] and asked == [(2, "ffn_v", 2)]
    del asked[:]
    assert sorted(_drop_path_masks(bb, 1, 2, False, False, dev)) == ["attn", "ffn", "keep"]
    assert asked == [(1, "attn", 2), (1, "ffn", 2)]
    del asked[:]
    bb.eval()
    assert all(_drop_path_masks(bb, i, 4, True, False, dev) is None for i in range(3)) and not asked
    bb.train()
    bb.drop_path_hook = lambda layer, site, B: torch.ones(B + 1)
    with pytest.raises(AssertionError):
        _drop_path_masks(bb, 1, 4, True, False, dev)


@pytest.mark.parametrize("name", ["A", "B"])
def test_build_model_and_the_fixtures_cases(name):
    """backbone=dict(..., drop_path_rate=r) through the model constructors; the state_dict is the reference's (keys and order:
    the fixture's seeded weight stream depends on it); the frozen clip_encoder has rate 0; the trainable backbone tensors are
    the fixture's gradient names"""
    z, _ = load_fixture("droppath")
    case = R.Case(z, name)
    hip = R.build_case(case)
    assert list(hip.state_dict()) == [str(k) for k in case["state_keys"]]
    fixture_state(case, case.cfg, hip)
    assert hip.backbone.drop_path_rate == case.spec["backbone"]["drop_path_rate"] and hip.backbone.dpr == list(case["dpr"])
    assert hip.clip_encoder.dpr == [0.0] * case.cfg["layers"]
    names = [str(n) for n in case["grad_names"] if str(n).startswith("backbone.")]
    tr = hip.backbone._trainable()
    assert sorted(n for n, p in hip.backbone.named_parameters() if any(p is q for q in tr)) == [n[len("backbone."):] for n in names]
    table = case.dp_masks("dp_masks")
    assert {k[0] for k in table} == {0, 1} and {k[2] for k in table} == set(R.SITES) and all(k[1] > 0 for k in table)
    assert all(m.numel() == 2 * case.cfg["B"] for m in table.values())
    # the coverage the generator promises, among the sites this project's step runs (not the last block's x path)
    live = [m for (f, l_, s_), m in table.items() if s_ == "ffn_v" or l_ < case.cfg["layers"] - 1]
    assert any(not m.any() for m in live) and any(m.all() for m in live)
    for s_ in R.SITES:
        ms = [m for (f, l_, s2), m in table.items() if s2 == s_ and (s_ == "ffn_v" or l_ < case.cfg["layers"] - 1)]
        assert any((m == 0).any() for m in ms) and any((m == 1).any() for m in ms)


def test_model_file_and_cfg_paths_reach_the_backbone():
    """cfg['model_args'] = dict(backbone=dict(drop_path_rate=...)) is how a run switches it on without a new model file"""
    import copy
    from semivl_amd.model.builder import builtin_model_cfg
    mcfg = copy.deepcopy(builtin_model_cfg("vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb"))["model"]
    assert mcfg["backbone"].get("drop_path_rate", 0.0) == 0.0       # the shipped recipes do not use it
    m = R.build_hip_prompt(dict(S=64, embed=64, layers=3, heads=1, out_indices=[0, 1, 3], channels=32, text_channels=32,
                                dec_heads=1, up=(32, 16), skip=(16, 16)), dict(drop_path_rate=0.2))
    assert m.backbone.dpr == [x.item() for x in torch.linspace(0, 0.2, 3)]
