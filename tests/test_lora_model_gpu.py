"""LoRA adapters of the CLIP ViT on the GPU (merged weights: ops.lora_merge in the forward, ops.lora_wgrad in the backward):
the two recipes of tests/golden/semivl_lora.npz through semivl_train_step against the reference's own step, with the
tolerances of test_vit_finetune_gpu.py::test_finetune_step_matches_reference_fixture (1e-3 on losses, 2e-3 on gradient
norms, 5e-3 relative max on full gradients); b_* = 0 is the base model bit for bit; nothing stale survives an optimizer step."""
import numpy as np
import pytest
import torch

import lora_ref as R
from golden_util import fixture_batch, fixture_fp_masks, fixture_state, load_fixture, seeded_state

pytestmark = pytest.mark.gpu

CFG = dict(conf_thresh=0.95, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
           maskclip_consistency_lambda=[0.1, 0])


@pytest.fixture(scope="module")
def fx():
    return load_fixture("lora")


def _model(fx, name, dev):
    z, c = fx
    case = R.Case(z, name)
    hip = R.build_case(c, case)
    hip.load_state_dict(fixture_state(case, c, hip), strict=True)
    return hip.to(dev), case


def _step(hip, case, c, dev, optimizer=None):
    from semivl_amd.train import LOSS_NAMES, semivl_train_step
    batch = {k: v.to(dev) for k, v in fixture_batch(case, c).items()}
    masks = [m.to(dev) for m in fixture_fp_masks(case, c)]
    iters, total = [int(v) for v in case["iters"]]
    hip.train()
    losses = semivl_train_step(hip, batch, iters, total, dict(CFG, conf_thresh=c["conf_thresh"]), optimizer=optimizer,
                               fp_masks=masks)
    return dict(zip(LOSS_NAMES, losses.cpu().numpy()))


def _check_grads(grads, case, what):
    """norms of every gradient and the full adapter gradients against the fixture (the ft test's tolerances)"""
    n_full = 0
    for k, g in grads.items():
        ref = case["gnorm/" + k]
        floor = 1e-5 if k == "decode_head.head.bias" else 1e-7
        assert abs(g.norm().item() - ref[0]) < 2e-3 * ref[0] + floor, f"{what}: grad norm of {k}: {g.norm().item()} vs {ref[0]}"
        if ("grad/" + k) in case.files:
            full = case["grad/" + k]
            e = np.abs(g.cpu().numpy() - full).max() / max(np.abs(full).max(), 1e-5)
            assert e < 5e-3, f"{what}: grad of {k}: rel max err {e}"
            n_full += 1
    return n_full


def _fixture_step(fx, name, dev):
    hip, case = _model(fx, name, dev)
    losses = _step(hip, case, fx[1], dev)
    for k, v in losses.items():
        assert abs(v - float(case[k])) < 1e-3 * max(1.0, abs(float(case[k]))), (k, v, float(case[k]))
    grads = {k: p.grad for k, p in hip.named_parameters() if p.grad is not None}
    assert sorted(grads) == [str(s) for s in case["grad_names"]]
    n_full = _check_grads(grads, case, name)
    assert n_full == sum(".lora." in k for k in grads) > 0
    return hip, grads


def test_lora_only_step_matches_reference_fixture(fx, dev):
    """case A: adapters on layers 0 (both paths) and 2 (the v-only last block), r = 4, s = 2, 'qkvo'; the base stays frozen"""
    hip, grads = _fixture_step(fx, "A", dev)
    assert all(".lora." in k for k in grads if k.startswith("backbone."))
    a = hip.backbone.layers[0].attn.attn
    assert a.in_proj_weight.grad is None and a.out_proj.weight.grad is None and a.in_proj_bias.grad is None
    for t in "qk":      # the v-only block's q / k adapters: all-zero gradients, like the reference's
        assert not grads[f"backbone.layers.2.lora.a_{t}.weight"].any() and not grads[f"backbone.layers.2.lora.b_{t}.weight"].any()


def test_lora_next_to_trained_projections_matches_reference_fixture(fx, dev):
    """case B: adapters on layer 1, r = 3, s = 0.5, 'qv', next to the ftap tensors (attention projections, pos_embed)"""
    _, grads = _fixture_step(fx, "B", dev)
    assert "backbone.layers.1.attn.attn.in_proj_weight" in grads and "backbone.pos_embed" in grads


@pytest.mark.parametrize("name", ["A", "B"])
def test_arena_sinks_match_reference_fixture(fx, dev, name):
    """the same step with main_grad sinks (an optimizer's arena): the two encoder backwards of the step accumulate into
    them, a frozen base projection has no sink and gets no gradient"""
    from semivl_amd.optim import FusedAdamW
    hip, case = _model(fx, name, dev)
    opt = FusedAdamW(hip, dict(type="AdamW", lr=1e-4, weight_decay=0.01))
    opt.zero_grad()
    _step(hip, case, fx[1], dev)
    opt._fold_autograd_grads()
    torch.cuda.synchronize()
    names = [str(s) for s in case["grad_names"]]
    grads = {k: p.main_grad for k, p in hip.named_parameters() if getattr(p, "main_grad", None) is not None and k in names}
    assert sorted(k for k, p in hip.backbone.named_parameters() if getattr(p, "main_grad", None) is not None) == \
        [k[len("backbone."):] for k in names if k.startswith("backbone.")]
    assert _check_grads(grads, case, name + " (arena)") > 0
    assert all(p.grad is None for p in hip.backbone.parameters())


def test_zero_b_is_the_base_model_bit_for_bit(fx, dev):
    """W + s * 0 @ A is W: same features as the model built with lora_layers=[]; and a model without adapters launches no
    lora_* kernel"""
    from semivl_amd import ops
    z, c = fx
    case = R.Case(z, "A")
    base = R.build_hip_lora(c, dict(lora_layers=[]), freeze_backbone=True, exclude_keys=["lora"])
    sd = seeded_state([(k, tuple(v.shape)) for k, v in base.state_dict().items()], c["seed"])
    base.load_state_dict(sd, strict=True)
    hip = R.build_case(c, case)
    res = hip.load_state_dict(sd, strict=False)     # the adapters keep their init: a_* random, b_* = 0
    assert res.missing_keys and all(".lora." in k for k in res.missing_keys) and not res.unexpected_keys
    base.to(dev).eval()
    hip.to(dev).eval()
    img = fixture_batch(case, c)["img_x"].to(dev)
    outs = {}
    try:
        for tag, m in (("base", base), ("lora", hip)):
            ops.PROFILE = {}
            with torch.no_grad():
                feats, glob = m.backbone.forward_tokens(img, need_global=True)
                feats2, _ = m.backbone.forward_tokens(img, need_global=False)
            torch.cuda.synchronize()
            outs[tag] = (list(feats) + [glob] + list(feats2), set(ops.PROFILE))
    finally:
        ops.PROFILE = None
    assert not any(k.startswith("lora_") for k in outs["base"][1])
    assert "lora_merge" in outs["lora"][1]
    assert len(outs["base"][0]) == len(outs["lora"][0]) > 2
    for a, b in zip(outs["base"][0], outs["lora"][0]):
        assert torch.equal(a, b)


def test_nothing_stale_after_an_optimizer_step(fx, dev):
    """two FusedAdamW steps: after the first, the stepped model's forward equals, bit for bit, the forward of a fresh model
    loaded from its state_dict (a merged weight cached across the step would differ); the frozen base is bit-unchanged"""
    from semivl_amd.optim import FusedAdamW
    z, c = fx
    hip, case = _model(fx, "A", dev)
    frozen = {k: p.detach().clone() for k, p in hip.backbone.named_parameters() if not p.requires_grad}
    before = {k: p.detach().clone() for k, p in hip.backbone.named_parameters() if p.requires_grad}
    assert frozen and before
    opt = FusedAdamW(hip, dict(type="AdamW", lr=1e-2, weight_decay=0.01))
    img = fixture_batch(case, c)["img_x"].to(dev)

    def feats(m):
        m.eval()
        with torch.no_grad():
            f, g = m.backbone.forward_tokens(img, need_global=True)
        return list(f) + [g]

    f0 = feats(hip)
    for it in range(2):
        _step(hip, case, c, dev, optimizer=opt)
        stepped = feats(hip)
        fresh = R.build_case(c, case)
        fresh.load_state_dict({k: v.detach().cpu() for k, v in hip.state_dict().items()}, strict=True)
        fresh.to(dev)
        for a, b in zip(stepped, feats(fresh)):
            assert torch.equal(a, b), f"step {it}"
        assert any(not torch.equal(a, b) for a, b in zip(stepped, f0)), "the step changed nothing"
        f0 = stepped
    now = dict(hip.backbone.named_parameters())
    assert all(torch.equal(v, now[k]) for k, v in frozen.items())
    moved = [k for k, v in before.items() if not torch.equal(v, now[k])]
    assert any(".lora.a_v." in k for k in moved) and any(".lora.b_o." in k for k in moved)


def test_lora_only_step_in_split_arithmetic(fx, dev):
    """case A under ops.set_gemm_emulation(6): the adapter gradients stay within the same tolerances"""
    from semivl_amd import ops
    hip, case = _model(fx, "A", dev)
    ops.set_gemm_emulation(6)
    try:
        losses = _step(hip, case, fx[1], dev)
    finally:
        ops.set_gemm_emulation(0)
    assert abs(losses["loss"] - float(case["loss"])) < 1e-3 * max(1.0, abs(float(case["loss"])))
    grads = {k: p.grad for k, p in hip.named_parameters() if p.grad is not None and ".lora." in k}
    assert len(grads) == 16 and _check_grads(grads, case, "A (mode 6)") == 16
