"""Deep visual prompts of the CLIP ViT on the GPU (ops.prompt_rows_fwd in the forward, ops.prompt_rows_bwd in the backward): the
two recipes of tests/golden/semivl_prompt.npz through semivl_train_step against the reference's own step (float64 fixture),
with the tolerances of test_vit_finetune_gpu.py / test_lora_model_gpu.py (1e-3 on losses, 2e-3 on gradient norms, 5e-3
relative max on full gradients); what a prompts-only backward launches; num_prompt_tokens=None is the model without the
argument; the optimizers leave prompt_norm.* alone; prompts next to LoRA; one encoder at the real row geometry (1035 rows)."""
import contextlib

import numpy as np
import pytest
import torch

import prompt_ref as R
from golden_util import fixture_batch, fixture_fp_masks, fixture_state, load_fixture, seeded_state

pytestmark = pytest.mark.gpu

CFG = dict(conf_thresh=0.95, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
           maskclip_consistency_lambda=[0.1, 0])
TRACED = ("matmul_tn", "matmul_tn_gelu", "matmul_tn_ln", "colsum", "reduce_slabs", "lora_wgrad", "prompt_rows_fwd",
          "prompt_rows_bwd")


@pytest.fixture(scope="module")
def fx():
    return load_fixture("prompt")


def _model(fx, name, dev):
    case = R.Case(fx[0], name)
    hip = R.build_case(case)
    hip.load_state_dict(fixture_state(case, case.cfg, hip), strict=True)
    return hip.to(dev), case


def _step(hip, case, dev, optimizer=None):
    from semivl_amd.train import LOSS_NAMES, semivl_train_step
    c = case.cfg
    batch = {k: v.to(dev) for k, v in fixture_batch(case, c).items()}
    masks = [m.to(dev) for m in fixture_fp_masks(case, c)]
    pm = case.prompt_masks()
    hip.backbone.prompt_mask_hook = None if pm is None else R.MaskQueue(list(pm), dev)
    iters, total = [int(v) for v in case["iters"]]
    hip.train()
    losses = semivl_train_step(hip, batch, iters, total, dict(CFG, conf_thresh=c["conf_thresh"]), optimizer=optimizer,
                               fp_masks=masks)
    if pm is not None:
        assert hip.backbone.prompt_mask_hook.i == len(pm)       # one mask per block and train-mode forward, none in eval mode
    return dict(zip(LOSS_NAMES, losses.cpu().numpy()))


def _check_grads(grads, case, what):
    """norms of every gradient and the full prompt gradients against the fixture (the ft / LoRA tests' tolerances)"""
    n_full = 0
    for k, g in grads.items():
        ref = case["gnorm/" + k]
        floor = 1e-5 if k == "decode_head.head.bias" else 1e-7
        assert abs(g.norm().item() - ref[0]) < 2e-3 * ref[0] + floor, f"{what}: grad norm of {k}: {g.norm().item()} vs {ref[0]}"
        if ("grad/" + k) in case.files:
            full = case["grad/" + k]
            e = np.abs(g.cpu().numpy() - full).max() / max(np.abs(full).max(), 1e-5)
            print(f"{what}: grad of {k}: rel max err {e:.2e}")
            assert e < 5e-3, f"{what}: grad of {k}: rel max err {e}"
            n_full += 1
    return n_full


def _fixture_step(fx, name, dev):
    hip, case = _model(fx, name, dev)
    losses = _step(hip, case, dev)
    for k, v in losses.items():
        assert abs(v - float(case[k])) < 1e-3 * max(1.0, abs(float(case[k]))), (k, v, float(case[k]))
    grads = {k: p.grad for k, p in hip.named_parameters() if p.grad is not None}
    assert sorted(grads) == [str(s) for s in case["grad_names"]]
    assert not any("prompt_norm" in k for k in grads) and bool(case["prompt_norm_grad_is_none"][0])
    assert _check_grads(grads, case, name) == 3
    return hip, grads


def test_prompts_only_step_matches_reference_fixture(fx, dev):
    """case A: 5 prompt rows, 1 head of 64 (the fused attention kernels on 70 rows), exclude_keys=['prompt'], no dropout"""
    hip, grads = _fixture_step(fx, "A", dev)
    assert sorted(k for k in grads if k.startswith("backbone.")) == sorted("backbone." + k for k in R.PROMPT_KEYS)
    a = hip.backbone.layers[0].attn.attn
    assert a.in_proj_weight.grad is None and a.out_proj.weight.grad is None and hip.backbone.prompt_norm.weight.grad is None


def test_prompts_next_to_trained_projections_with_dropout_matches_reference_fixture(fx, dev):
    """case B: 3 prompt rows, 4 heads of 16 (the generic attention path), next to the ftap tensors, prompt_dropout live with
    the fixture's recorded masks (per sample, in the reference's [x, w] row order)"""
    _, grads = _fixture_step(fx, "B", dev)
    assert "backbone.layers.1.attn.attn.in_proj_weight" in grads and "backbone.pos_embed" in grads


def test_prompts_only_step_in_split_arithmetic(fx, dev):
    """case A under ops.set_gemm_emulation(6): the same tolerances"""
    from semivl_amd import ops
    hip, case = _model(fx, "A", dev)
    ops.set_gemm_emulation(6)
    try:
        losses = _step(hip, case, dev)
    finally:
        ops.set_gemm_emulation(0)
    assert abs(losses["loss"] - float(case["loss"])) < 1e-3 * max(1.0, abs(float(case["loss"])))
    grads = {k: p.grad for k, p in hip.named_parameters() if p.grad is not None and "prompt" in k}
    assert len(grads) == 3 and _check_grads(grads, case, "A (mode 6)") == 3


# ------------------------------------------------------------------------------------------------ structure
@contextlib.contextmanager
def _traced():
    """(calls, profile): every call of the weight-gradient / prompt wrappers of semivl_amd.ops as (name, shape of its first
    tensor), and ops.PROFILE (the GEMM launches with their operand modes, the prompt_ families)"""
    from semivl_amd import ops
    calls, keep = [], {n: getattr(ops, n) for n in TRACED}

    def wrap(n, fn):
        def f(*a, **k):
            calls.append((n, tuple(next(t for t in a if torch.is_tensor(t)).shape)))
            return fn(*a, **k)
        return f

    for n, fn in keep.items():
        setattr(ops, n, wrap(n, fn))
    ops.PROFILE = {}
    try:
        yield calls, ops.PROFILE
    finally:
        ops.PROFILE = None
        for n, fn in keep.items():
            setattr(ops, n, fn)


def _a_mode(tag):
    """the A-operand mode of a profiled svl_gemm_f32 launch (ops.gemm's tag), None for the packed-planes GEMM"""
    if isinstance(tag[0], str):
        return tag[1] if tag[0] == "split_h2" else None
    return tag[0]


def _encoder_run(bb, img, cots, need_global=True):
    """forward_tokens + the backward of sum_j <feat_j, cots_j> -> (features + [global], {name: grad})"""
    for p in bb.parameters():
        p.grad = None
    feats, glob = bb.forward_tokens(img, need_global=need_global)
    sum((f * c).sum() for f, c in zip(feats, cots)).backward()
    torch.cuda.synchronize()
    return list(feats) + [glob], {k: p.grad for k, p in bb.named_parameters() if p.grad is not None}


def _case_encoder(fx, name, dev):
    hip, case = _model(fx, name, dev)
    c = case.cfg
    img = fixture_batch(case, c)["img_x"].to(dev)
    NP = (c["S"] // 16) ** 2
    cots = [t.to(dev) for t in R.seeded_cots([(c["B"], NP, 512 if o == c["layers"] else c["embed"]) for o in c["out_indices"]],
                                             c["seed"] + 400)]
    return hip, case, img, cots


def test_a_prompts_only_backward_launches_no_block_weight_gradient(fx, dev):
    """case A, the encoder alone: the only weight-gradient GEMM and column sum of the backward are the two of prompt_proj
    (15 = L * P rows: one pass, no slab reduction); the blocks launch none.  The prompt_ kernels: one expand and L - 1 in-place
    forwards, L backwards (the last one, block 0's, compacts)."""
    from semivl_amd import ops
    hip, case, img, cots = _case_encoder(fx, "A", dev)
    L, P, E = case.cfg["layers"], case.spec["backbone"]["num_prompt_tokens"], case.cfg["embed"]
    hip.train()
    with _traced() as (calls, prof):
        _, grads = _encoder_run(hip.backbone, img, cots)
    assert sorted(grads) == sorted(R.PROMPT_KEYS)
    assert [c for c in calls if not c[0].startswith("prompt_")] == [("matmul_tn", (L * P, E)), ("colsum", (L * P, E))]
    wg = [t[3] for fam in ("gemm", "gemm_bf16x") for t in prof.get(fam, ()) if _a_mode(t[3]) == ops.A_MC]
    assert len(wg) == 1 and L * P in wg[0]      # (A_MC: the A operand read transposed -- dY^T @ X, a weight gradient)
    fwd, bwd = [t[3] for t in prof["prompt_rows_fwd"]], [t[3] for t in prof["prompt_rows_bwd"]]
    assert [t[4] for t in fwd] == [True] + [False] * (L - 1) and [t[4] for t in bwd] == [False] * (L - 1) + [True]


def test_ftap_without_prompts_still_launches_its_weight_gradients(fx, dev):
    from golden_util import build_hip
    _, case, img, cots = _case_encoder(fx, "A", dev)
    c = case.cfg
    hip = build_hip(c)
    hip.freeze(hip.backbone, exclude_keys=["attn", "pos_embed"])
    hip.to(dev).train()
    with _traced() as (calls, prof):
        _, grads = _encoder_run(hip.backbone, img, cots)
    L = c["layers"]
    assert not any(n.startswith("prompt_") for n, _ in calls) and not any(k.startswith("prompt_") for k in prof)
    assert sum(n == "matmul_tn" for n, _ in calls) >= 2 * L and sum(n == "colsum" for n, _ in calls) >= 2 * L
    assert all(f"layers.{i}.attn.attn.in_proj_weight" in grads and f"layers.{i}.attn.attn.out_proj.bias" in grads for i in range(L))


def test_no_prompts_is_the_model_without_the_argument(fx, dev):
    """num_prompt_tokens=None against a model built without the argument, both recipes (ftap, and everything frozen but
    pos_embed -- the one recipe whose launches this change touches: its blocks' discarded weight gradients are gone): the
    same calls, the same GEMM launches, bit-equal outputs and gradients"""
    from golden_util import build_hip
    _, case, img, cots = _case_encoder(fx, "A", dev)
    c = case.cfg
    ref = build_hip(c)
    sd = seeded_state([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], c["seed"])
    new = R.build_hip_prompt(c, dict(num_prompt_tokens=None))
    runs = {}
    for tag, m in (("without", ref), ("none", new)):
        m.load_state_dict(sd, strict=True)
        m.to(dev).train()
        for keys in (["attn", "pos_embed"], ["pos_embed"]):
            m.freeze(m.backbone, exclude_keys=keys)
            m.backbone.__dict__.pop("_ruled", None)
            with _traced() as (calls, prof):
                outs, grads = _encoder_run(m.backbone, img, cots)
            runs[tag, len(keys)] = (calls, {k: [t[3] for t in v] for k, v in prof.items()}, outs, grads)
    for n in (1, 2):
        a, b = runs["without", n], runs["none", n]
        assert a[0] == b[0] and a[1] == b[1] and len(a[1].get("gemm", ())) + len(a[1].get("gemm_bf16x", ())) > 10
        assert all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and len(a[2]) == 4
        assert sorted(a[3]) == sorted(b[3]) and all(torch.equal(a[3][k], b[3][k]) for k in a[3])
    assert not any(n.startswith("prompt_") for n, _ in runs["none", 2][0])
    assert not any(n in ("matmul_tn", "colsum") for n, _ in runs["none", 1][0]) and list(runs["none", 1][3]) == ["pos_embed"]


# ------------------------------------------------------------------------------------------------ the encoder against prompt_ref
def _against_ref(bb, sd, img, cots, what, masks=None, **kw):
    """the product encoder's features and prompt gradients against encoder_ref in float64: 1e-3 (features), 2e-3 (gradient
    norms), 5e-3 (full gradients), each relative to the tensor's max-abs / norm"""
    dev = img.device
    bb.prompt_mask_hook = None if masks is None else R.MaskQueue(list(masks), dev)
    outs, grads = _encoder_run(bb, img, cots)
    feats, glob, rg = R.encoder_prompt_grads(sd, img.cpu(), [c.cpu() for c in cots], heads=bb.num_heads,
                                             out_indices=bb.out_indices, P=bb.num_prompt_tokens, masks=masks, eps=bb.eps)
    worst = [0.0, 0.0, 0.0]
    for got, want in zip(outs, feats + [glob]):
        worst[0] = max(worst[0], ((got.double().cpu() - want).abs().max() / want.abs().max()).item())
    for k in R.PROMPT_KEYS:
        g = grads[k].double().cpu()
        assert rg[k].abs().max() > 0
        worst[1] = max(worst[1], abs(g.norm().item() / rg[k].norm().item() - 1))
        worst[2] = max(worst[2], ((g - rg[k]).abs().max() / rg[k].abs().max()).item())
    print(f"{what}: features {worst[0]:.2e}, prompt gradient norms {worst[1]:.2e}, prompt gradients rel max {worst[2]:.2e}")
    assert worst[0] < 1e-3 and worst[1] < 2e-3 and worst[2] < 5e-3
    return outs, grads


@pytest.mark.parametrize("name", ["A", "B"])
def test_encoder_matches_prompt_ref_and_each_layers_prompts_matter(fx, dev, name):
    """gradient isolation: the product's prompt gradients are those of the float64 restatement, in which block i's prompt rows
    are discarded after the block -- a gradient leaking from block i + 1's prompt rows into block i would be an O(1) error on
    deep_prompt_embeddings[i]; and every layer's prompts reach the output"""
    hip, case, img, cots = _case_encoder(fx, name, dev)
    hip.train()
    bb = hip.backbone
    sd = {k: v.detach().cpu() for k, v in bb.state_dict().items()}
    masks = case.prompt_masks("enc_masks")
    outs, grads = _against_ref(bb, sd, img, cots, f"case {name}", masks=masks)
    # (the last block's prompts reach only its x path, i.e. the global embedding, which carries no gradient: exactly zero, in
    # the restatement too)
    nz = [bool(grads["deep_prompt_embeddings"][i].any()) for i in range(case.cfg["layers"])]
    assert nz == [True] * (case.cfg["layers"] - 1) + [False]
    bb.prompt_mask_hook = None
    hip.eval()
    with torch.no_grad():
        base = bb.forward_tokens(img, need_global=True)
        for i in range(case.cfg["layers"]):
            bb.deep_prompt_embeddings[i] += 0.5
            out = bb.forward_tokens(img, need_global=True)
            bb.deep_prompt_embeddings[i] -= 0.5
            changed = [not torch.equal(a, b) for a, b in zip(list(base[0]) + [base[1]], list(out[0]) + [out[1]])]
            # (block 0's v path sees no attention: the first feature cannot depend on any prompt)
            assert not changed[0] and (all(changed[1:]) if i == 0 else any(changed[1:])), (i, changed)


def test_prompts_next_to_lora(fx, dev):
    """prompts + lora_layers=[1] + exclude_keys=['lora', 'prompt'], B = 1: the prompt gradients against the restatement run
    on the merged weights W + s * B @ A; the adapters get non-zero, finite gradients; two runs agree bit for bit"""
    _, case, img, cots = _case_encoder(fx, "A", dev)
    c = case.cfg
    hip = R.build_hip_prompt(c, dict(num_prompt_tokens=2, lora_layers=[1], lora_r=3, lora_scaling=0.5, lora_targets="qkvo"),
                             freeze_backbone=True, exclude_keys=["lora", "prompt"])
    hip.load_state_dict(seeded_state([(k, tuple(v.shape)) for k, v in hip.state_dict().items()], c["seed"] + 1), strict=True)
    hip.to(dev).train()
    bb = hip.backbone
    sd = {k: v.detach().cpu().double() for k, v in bb.state_dict().items()}
    E = c["embed"]
    for t, (key, rows) in dict(q=("in_proj_weight", 0), k=("in_proj_weight", E), v=("in_proj_weight", 2 * E),
                               o=("out_proj.weight", 0)).items():
        sd[f"layers.1.attn.attn.{key}"][rows:rows + E] += 0.5 * sd[f"layers.1.lora.b_{t}.weight"] @ sd[f"layers.1.lora.a_{t}.weight"]
    img, cots = img[:1].contiguous(), [t[:1].contiguous() for t in cots]
    outs, grads = _against_ref(bb, {k: v for k, v in sd.items() if ".lora." not in k}, img, cots, "prompts + LoRA")
    lora = [k for k in grads if ".lora." in k]
    assert len(lora) == 8 and sorted(grads) == sorted(lora + list(R.PROMPT_KEYS))
    assert all(torch.isfinite(grads[k]).all() and grads[k].abs().max() > 0 for k in grads)
    outs2, grads2 = _encoder_run(bb, img, cots)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2)) and all(torch.equal(grads[k], grads2[k]) for k in grads)


@pytest.mark.parametrize("mode", [0, 6])
def test_real_row_geometry(dev, mode):
    """E = 768, 12 heads, 2 layers, S = 512, P = 10, B = 1: 1035 rows per image, a GEMM row count and an attention tail no
    other test has; forward and backward against the float64 restatement (on the CPU) in exact and in split arithmetic"""
    from semivl_amd import ops
    from semivl_amd.model.vit import MaskClipVisionTransformer
    torch.manual_seed(3)
    bb = MaskClipVisionTransformer(img_size=(512, 512), patch_size=16, patch_bias=False, embed_dims=768, num_layers=2,
                                   num_heads=12, out_indices=[0, 2], pre_norm=True, final_norm=True, return_clip_embed=True,
                                   return_qkv=True, norm_cfg=dict(type="LN", eps=1e-6), num_prompt_tokens=10)
    bb.load_state_dict(seeded_state([(k, tuple(v.shape)) for k, v in bb.state_dict().items()], 21), strict=True)
    for n, p in bb.named_parameters():
        p.requires_grad = "prompt" in n
    sd = {k: v.detach().clone() for k, v in bb.state_dict().items()}
    bb.to(dev).train()
    g = torch.Generator().manual_seed(4)
    img = torch.randn(1, 3, 512, 512, generator=g).to(dev)
    cots = [t.to(dev) for t in R.seeded_cots([(1, 1024, 768), (1, 1024, 512)], 5)]
    ops.set_gemm_emulation(mode)
    try:
        _, grads = _against_ref(bb, sd, img, cots, f"1035 rows, mode {mode}")
    finally:
        ops.set_gemm_emulation(0)
    assert sorted(grads) == sorted(R.PROMPT_KEYS)


# ------------------------------------------------------------------------------------------------ optimizers
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_optimizers_move_the_prompts_and_leave_prompt_norm_alone(fx, dev, which):
    """two steps of FusedAdamW (weight decay 0.01, no custom keys) / FusedSGD.original: the three prompt tensors move;
    prompt_norm.* -- requires_grad like the reference's, never given a gradient -- and every frozen tensor are bit-unchanged
    (no update, no weight decay); after each step the model's forward equals a fresh model's loaded from its state_dict;
    zero_grad leaves nothing behind"""
    from semivl_amd.optim import FusedAdamW, FusedSGD
    hip, case = _model(fx, "A", dev)
    bb = hip.backbone
    assert bb.prompt_norm.weight.requires_grad and bb.prompt_norm.bias.requires_grad
    opt = (FusedAdamW(hip, dict(type="AdamW", lr=1e-2, weight_decay=0.01)) if which == "adamw" else
           FusedSGD.original(hip, 1e-3, 10.0))
    fixed = {k: p.detach().clone() for k, p in bb.named_parameters() if not p.requires_grad or "prompt_norm" in k}
    before = {k: p.detach().clone() for k, p in bb.named_parameters() if k in R.PROMPT_KEYS}
    assert len(fixed) > 30 and len(before) == 3
    assert all(getattr(p, "main_grad", None) is None for k, p in bb.named_parameters() if k in fixed)
    img = fixture_batch(case, case.cfg)["img_x"].to(dev)

    def feats(m):
        m.eval()
        with torch.no_grad():
            f, g = m.backbone.forward_tokens(img, need_global=True)
        return list(f) + [g]

    f0 = feats(hip)
    for it in range(2):
        _step(hip, case, dev, optimizer=opt)
        stepped = feats(hip)
        fresh = R.build_case(case)
        fresh.load_state_dict({k: v.detach().cpu() for k, v in hip.state_dict().items()}, strict=True)
        for a, b in zip(stepped, feats(fresh.to(dev))):
            assert torch.equal(a, b), f"step {it}"
        assert any(not torch.equal(a, b) for a, b in zip(stepped, f0)), "the step changed nothing"
        f0 = stepped
    now = dict(bb.named_parameters())
    assert all(torch.equal(v, now[k]) for k, v in fixed.items())
    assert all(not torch.equal(v, now[k]) for k, v in before.items())
    assert all(p.grad is None for p in bb.parameters())
    opt.zero_grad()
    torch.cuda.synchronize()
    assert not opt.g.any()
