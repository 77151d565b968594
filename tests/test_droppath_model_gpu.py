"""Stochastic depth of the CLIP ViT on the GPU (ops.droppath_add in the forward, ops.droppath_scale in the backward): the two
recipes of tests/golden/semivl_droppath.npz -- full fine-tuning, and LoRA + prompts + trained projections -- through the encoder
alone and through semivl_train_step against the reference's own run (float64 fixture) with the fixture's masks injected through
backbone.drop_path_hook, in exact and in split GEMM arithmetic, with the limits of test_prompt_model_gpu.py (1e-3 on losses and
features, 2e-3 on gradient norms, 5e-3 relative max on full gradients); the [x, w] row order of injected masks; rate 0 and eval
mode are the model without the option; draws are {0, 1} and follow torch.manual_seed.  Every test builds a model with
drop_path_rate > 0, which the constructor refused before this option existed."""
import contextlib

import numpy as np
import pytest
import torch

import droppath_ref as R
from golden_util import build_hip, fixture_batch, fixture_fp_masks, fixture_state, load_fixture, seeded_state

pytestmark = pytest.mark.gpu

CFG = dict(conf_thresh=0.95, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
           maskclip_consistency_lambda=[0.1, 0])


@pytest.fixture(scope="module")
def fx():
    return load_fixture("droppath")


@contextlib.contextmanager
def _mode(mode):
    from semivl_amd import ops
    ops.set_gemm_emulation(mode)
    try:
        yield
    finally:
        ops.set_gemm_emulation(0)


@contextlib.contextmanager
def _spy():
    """every call of ops.droppath_add / ops.droppath_scale as (name, mask on the host, keep), and ops.PROFILE"""
    from semivl_amd import ops
    calls, keep = [], {n: getattr(ops, n) for n in ("droppath_add", "droppath_scale")}

    def wrap(n, fn):
        j = 2 if n == "droppath_add" else 1     # (branch, resid, mask, keep, ...) / (dout, mask, keep, ...)

        def f(*a, **k):
            calls.append((n, a[j].detach().cpu().clone(), a[j + 1]))
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


def _model(fx, name, dev):
    case = R.Case(fx[0], name)
    hip = R.build_case(case)
    hip.load_state_dict(fixture_state(case, case.cfg, hip), strict=True)
    return hip.to(dev), case


def _step(hip, case, dev, table=None):
    from semivl_amd.train import LOSS_NAMES, semivl_train_step
    c = case.cfg
    batch = {k: v.to(dev) for k, v in fixture_batch(case, c).items()}
    masks = [m.to(dev) for m in fixture_fp_masks(case, c)]
    hook = hip.backbone.drop_path_hook = R.MaskTable(case.dp_masks("dp_masks") if table is None else table, dev)
    iters, total = [int(v) for v in case["iters"]]
    hip.train()
    losses = semivl_train_step(hip, batch, iters, total, dict(CFG, conf_thresh=c["conf_thresh"]), fp_masks=masks)
    assert hip.backbone.drop_path_hook is hook
    # one request per live site and train-mode forward (none in the eval-mode passes): blocks 1 and 2, the last block's x
    # path is not computed in the step
    L = c["layers"]
    want = [(f, i, s) for f in (0, 1) for i in range(1, L) for s in (("ffn_v", "attn", "ffn") if i < L - 1 else ("ffn_v",))]
    assert hook.used == want, hook.used
    return dict(zip(LOSS_NAMES, losses.cpu().numpy()))


def _check_grads(grads, case, what, names=None):
    """norms of every gradient and the fixture's full gradients (the prompt / ft / LoRA tests' tolerances)"""
    n_full, worst = 0, [0.0, 0.0]
    for k, g in grads.items():
        if names is not None and k not in names:
            continue
        ref = case["gnorm/" + k]
        floor = 1e-5 if k == "decode_head.head.bias" else 1e-7
        worst[0] = max(worst[0], abs(g.norm().item() - ref[0]) / max(ref[0], 1e-30) if ref[0] > 1e-4 else 0.0)
        assert abs(g.norm().item() - ref[0]) < 2e-3 * ref[0] + floor, f"{what}: grad norm of {k}: {g.norm().item()} vs {ref[0]}"
        if ("grad/" + k) in case.files:
            full = case["grad/" + k]
            e = np.abs(g.cpu().numpy() - full).max() / max(np.abs(full).max(), 1e-5)
            print(f"{what}: grad of {k}: rel max err {e:.2e}")
            worst[1] = max(worst[1], e)
            assert e < 5e-3, f"{what}: grad of {k}: rel max err {e}"
            n_full += 1
    print(f"{what}: worst gradient norm distance {worst[0]:.2e}, worst full gradient rel max err {worst[1]:.2e}")
    return n_full


@pytest.mark.parametrize("mode", [0, 6])
@pytest.mark.parametrize("name", ["A", "B"])
def test_step_matches_reference_fixture(fx, dev, name, mode):
    """A: every backbone tensor trains, 1 head of 64 (the fused attention kernels), rates 0, 0.25, 0.5.  B: 4 heads of 16,
    adapters in blocks 1 and 2, 3 prompt rows (a sample's 68 rows take its one draw), rates 0, 0.2, 0.4, disable_dropout=True:
    stochastic depth is live all the same.  The masks come in the reference's [x, w] row order.  Mode 0: every loss, every
    gradient's norm, the fixture's full gradients; mode 6 (as the prompt test does): the loss and the fixture's full gradients
    with their norms."""
    hip, case = _model(fx, name, dev)
    assert hip.backbone.disable_dropout and hip.disable_dropout
    with _mode(mode):
        losses = _step(hip, case, dev)
    for k, v in losses.items():
        d = abs(v - float(case[k])) / max(1.0, abs(float(case[k])))
        print(f"{name} mode {mode}: {k} {v:.6f} vs {float(case[k]):.6f} ({d:.2e})")
        if mode == 0 or k == "loss":
            assert d < 1e-3, (k, v, float(case[k]))
    grads = {k: p.grad for k, p in hip.named_parameters() if p.grad is not None}
    assert sorted(grads) == [str(s) for s in case["grad_names"]]
    full = case.spec["full"]
    assert _check_grads(grads, case, f"{name} mode {mode}", names=None if mode == 0 else full) == len(full)


def test_injected_masks_reach_the_blocks_in_w_x_order(fx, dev):
    """the first forward of the step runs on [w, x] where the reference runs on [x, w]: a mask injected in the reference's
    order reaches the kernels with its halves swapped; the second forward ([s1, s2] in both) takes it as it is"""
    hip, case = _model(fx, "A", dev)
    B = case.cfg["B"]
    table = case.dp_masks("dp_masks")
    with _spy() as (calls, _):
        _step(hip, case, dev)
    adds = [m for n, m, _ in calls if n == "droppath_add"]
    order = [(1, "ffn_v"), (1, "attn"), (1, "ffn"), (2, "ffn_v")]
    assert len(adds) == 8
    for j, (i, s) in enumerate(order):
        m0, m1 = table[0, i, s], table[1, i, s]
        assert torch.equal(adds[j], torch.cat((m0[B:], m0[:B]))) and torch.equal(adds[4 + j], m1)
    assert any(not torch.equal(table[0, i, s][B:], table[0, i, s][:B]) for i, s in order)     # (so the order is visible)
    # the backward scales with the masks of the forward it belongs to (the step's one backward runs both graphs)
    scal = [m for n, m, _ in calls if n == "droppath_scale"]
    assert len(scal) == 8 and sorted(m.tolist() for m in scal) == sorted(m.tolist() for m in adds)
    assert {k for _, _, k in calls} == {0.75, 0.5}


# ------------------------------------------------------------------------------------------------ the encoder alone
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


@pytest.mark.parametrize("mode", [0, 6])
@pytest.mark.parametrize("name", ["A", "B"])
def test_encoder_matches_reference_fixture(fx, dev, name, mode):
    """the encoder alone in train mode with the global embedding (so the last block's x path and its two sites run): features
    1e-3, gradient norms 2e-3, full gradients 5e-3, each relative to the fixture tensor's max-abs / norm"""
    hip, case, img, cots = _case_encoder(fx, name, dev)
    hip.train()
    bb = hip.backbone
    hook = bb.drop_path_hook = R.MaskTable(case.dp_masks("enc_masks"), dev)
    with _mode(mode):
        outs, grads = _encoder_run(bb, img, cots)
    assert hook.used == [(0, i, s) for i in (1, 2) for s in ("ffn_v", "attn", "ffn")]
    worst = [0.0, 0.0, 0.0]
    for j, got in enumerate(outs[:-1]):
        want = case[f"enc/feat{j}"]
        g = (got[0, :, ::8] if got.shape[-1] == 512 else got[0]).detach().double().cpu().numpy()
        worst[0] = max(worst[0], np.abs(g - want).max() / np.abs(want).max())
    worst[0] = max(worst[0], np.abs(outs[-1].detach().double().cpu().numpy() - case["enc/glob"]).max() / np.abs(case["enc/glob"]).max())
    zero = []
    for k in case.spec["enc_keys"]:
        want, g = case["enc/grad/" + k], grads[k].double().cpu().numpy()
        if not np.abs(want).max() > 0:      # behind a site that dropped every sample
            assert not g.any(), k
            zero.append(k)
            continue
        worst[1] = max(worst[1], abs(np.linalg.norm(g) / np.linalg.norm(want) - 1))
        worst[2] = max(worst[2], np.abs(g - want).max() / np.abs(want).max())
    print(f"case {name} mode {mode}: features {worst[0]:.2e}, gradient norms {worst[1]:.2e}, gradients rel max {worst[2]:.2e}; "
          f"exactly zero: {zero}")
    assert len(zero) <= 1 and worst[0] < 1e-3 and worst[1] < 2e-3 and worst[2] < 5e-3


# ------------------------------------------------------------------------------------------------ no-op guarantees
def test_rate_zero_and_eval_mode_are_the_model_without_the_option(fx, dev):
    """drop_path_rate=0.0 in train mode (forward and backward) and drop_path_rate=0.3 in eval mode against a model built without
    the argument: bit-equal features (and gradients at rate 0); the rate-0 model calls no droppath wrapper and launches no
    droppath kernel, the eval-mode forward of the 0.3 model neither"""
    _, case, img, cots = _case_encoder(fx, "A", dev)
    c = case.cfg
    ref = build_hip(c)
    sd = seeded_state([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], c["seed"])
    zero, some = R.build_hip_prompt(c, dict(drop_path_rate=0.0)), R.build_hip_prompt(c, dict(drop_path_rate=0.3))
    for m in (ref, zero, some):
        m.load_state_dict(sd, strict=True)
        m.freeze(m.backbone, exclude_keys=[""])         # every backbone tensor trains
        m.to(dev)
    ref.train()
    zero.train()
    base, gbase = _encoder_run(ref.backbone, img, cots)
    with _spy() as (calls, prof):
        outs, grads = _encoder_run(zero.backbone, img, cots)
    assert not calls and not any(k.startswith("droppath") for k in prof) and len(prof) >= 2     # (the profile saw the run: GEMM and attention families)
    assert len(base) == 4 and all(torch.equal(a, b) for a, b in zip(base, outs))
    assert sorted(gbase) == sorted(grads) and len(grads) == 44 and all(torch.equal(gbase[k], grads[k]) for k in grads)
    ref.eval()
    some.eval()
    asked = []
    some.backbone.drop_path_hook = lambda *a: asked.append(a)
    with torch.no_grad(), _spy() as (calls, prof):
        e0 = ref.backbone.forward_tokens(img, need_global=True)
        e1 = some.backbone.forward_tokens(img, need_global=True)
    assert not calls and not asked and not any(k.startswith("droppath") for k in prof)
    assert all(torch.equal(a, b) for a, b in zip(list(e0[0]) + [e0[1]], list(e1[0]) + [e1[1]]))
    # and the same model in train mode does drop: the option is live
    some.train()
    some.backbone.drop_path_hook = None
    torch.manual_seed(0)
    with _spy() as (calls, prof):
        _encoder_run(some.backbone, img, cots)
    # (6 sites in the forward; the last block's x path feeds only the global embedding, which carries no gradient: 4 in the backward)
    assert [n for n, _, _ in calls].count("droppath_add") == 6 and [n for n, _, _ in calls].count("droppath_scale") == 4
    assert len(prof["droppath_add"]) == 6 and len(prof["droppath_scale"]) == 4


def test_draws_are_zero_one_and_follow_the_seed(fx, dev):
    """without a hook: each live site's mask holds only 0 and 1, one value per sample; two train-mode forward + backward runs
    under one torch.manual_seed agree bit for bit (masks, features, gradients); another seed draws other masks"""
    hip, case, img, cots = _case_encoder(fx, "A", dev)
    bb = hip.backbone
    img, cots = torch.cat([img] * 4), [torch.cat([t] * 4) for t in cots]      # 8 samples: masks with room to differ
    hip.train()
    runs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        with _spy() as (calls, _):
            outs, grads = _encoder_run(bb, img, cots)
        masks = [m for n, m, _ in calls if n == "droppath_add"]
        assert len(masks) == 6 and all(m.shape == (8,) and bool(((m == 0) | (m == 1)).all()) for m in masks)
        assert [k for n, _, k in calls if n == "droppath_add"] == [0.75] * 3 + [0.5] * 3
        runs.append((masks, outs, grads))
    a, b, c_ = runs
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert sorted(a[2]) == sorted(b[2]) and len(a[2]) == 44 and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert any(not torch.equal(x, y) for x, y in zip(a[0], c_[0]))
    assert any(not torch.equal(x, y) for x, y in zip(a[0][:-1], a[0][1:]))      # sites draw independently
