"""The OHEM supervised criterion on the GPU: the exact radix select against torch.kthvalue, the two target-probability
kernels against float64, ops.ohem_target / ProbOhemCrossEntropy2d against the reference's own criterion
(ohem_cases.npz), and the training step with cfg['criterion'] = 'OHEM' against the reference loop (semivl_ohem.npz) and
against a plain cross-entropy step on the relabelled map."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import build_hip, fixture_batch, fixture_fp_masks, fixture_state, load_fixture

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = dict(conf_thresh=0.95, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
           maskclip_consistency_lambda=[0.1, 0])


def to_dev(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _data(kind, n, dev):
    g = torch.Generator(device=dev).manual_seed(n + len(kind))
    if kind == "uniform":
        return torch.rand(n, device=dev, generator=g)
    if kind == "equal":
        return torch.full((n,), 0.3125, device=dev)
    if kind == "two":
        return torch.where(torch.rand(n, device=dev, generator=g) < 0.4, 0.25, 0.75)
    x = torch.rand(n, device=dev, generator=g)        # many exact 0.0 and 1.0
    r = torch.rand(n, device=dev, generator=g)
    return torch.where(r < 0.3, 0.0, torch.where(r > 0.6, 1.0, x))


@pytest.mark.parametrize("kind", ["uniform", "equal", "two", "zeros_ones"])
@pytest.mark.parametrize("n", [1, 7, 4095, 65537, 16 * 512 * 512, 8 * 801 * 801])
def test_kth_smallest_matches_kthvalue(dev, n, kind):
    from semivl_amd import ops
    x = _data(kind, n, dev).float().contiguous()
    for k in sorted({1, max(1, n // 2), n}):
        got = ops.kth_smallest(x, k)
        ref = torch.kthvalue(x, k).values
        assert torch.equal(got.view(-1).view(torch.int32), ref.view(1).view(torch.int32)), (n, k, kind, got.item(), ref.item())


def _target(B, H, W, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, N, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.2] = 255
    return t.to(dev)


def _p64(full, t):
    valid = t != 255
    p = F.softmax(full.double(), dim=1).gather(1, (t * valid).unsqueeze(1)).squeeze(1)
    return torch.where(valid, p, torch.ones_like(p))


@pytest.mark.parametrize("N", [5, 21])
@pytest.mark.parametrize("align", [False, True])
def test_target_prob_kernels_match_fp64(dev, N, align):
    from semivl_amd import ops
    g = torch.Generator().manual_seed(7 + N)
    B, h, w, H, W = 2, 16, 12, 64, 48
    low = torch.randn(B, N, h, w, generator=g).to(dev)     # (|logit| ~ 1: the fp32 rounding of the logits themselves stays << 1e-6 in p)
    t = _target(B, H, W, N, dev, N)
    full64 = F.interpolate(low.double(), size=(H, W), mode="bilinear", align_corners=align)
    ref = _p64(full64, t)
    got_up = ops.target_prob(low, t, up=(H, W, align))
    got_full = ops.target_prob(full64.float().contiguous(), t)
    for got in (got_up, got_full):
        assert got.shape == (B, H, W)
        assert (got.double() - ref).abs().max().item() < 1e-6
        assert torch.equal(got[t == 255], torch.ones_like(got[t == 255]))


def _cases():
    z = np.load(os.path.join(GOLDEN, "ohem_cases.npz"))
    return z, int(z["num_cases"])


@pytest.mark.parametrize("path", ["up", "full"])
def test_ohem_target_matches_reference_cases(dev, path):
    from semivl_amd import ops
    from semivl_amd.train import ProbOhemCrossEntropy2d
    z, nc = _cases()
    for i in range(nc):
        pre = f"c{i}/"
        name = str(z[pre + "name"])
        H, W, align = (int(v) for v in z[pre + "geom"])
        align = bool(align)
        low = torch.from_numpy(z[pre + "logits"]).to(dev)
        t = torch.from_numpy(z[pre + "target"].astype(np.int64)).to(dev)
        thresh, mk = float(z[pre + "thresh"]), int(z[pre + "min_kept"])
        ref_relabel, ref_loss, ref_grad = z[pre + "relabel"], float(z[pre + "loss"]), z[pre + "grad"]
        if path == "up":
            cnt = ops.zeros(1, dtype=torch.int64, device=dev)
            rel = ops.ohem_target(low, t, thresh, mk, up=(H, W, align), counts_out=cnt)
            kept = int(cnt.item())
            assert kept == int((rel != 255).sum().item()), name
            # the step's cross entropy on the relabelled map: mean over the kept pixels, gradient at the low resolution
            gscale = torch.tensor([1.0 / max(kept, 1), 0.0], device=dev)
            dl = torch.empty_like(low)
            sums = ops.ce_up_fused(low, H, W, align, rel, True, dlogits=dl, gscale=gscale)
            loss = (sums[0] / sums[3]).item()
            grad = dl.cpu().numpy()
        else:
            x = low.clone().requires_grad_(True)
            crit = ProbOhemCrossEntropy2d(255, thresh=thresh, min_kept=mk)
            full = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=align)
            rel = crit.relabel(full, t)
            lt = crit(full, t)
            lt.backward()
            loss, grad = lt.item(), x.grad.cpu().numpy()
        assert np.array_equal(rel.cpu().numpy().astype(np.uint8), ref_relabel), (name, path)
        assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (name, path, loss, ref_loss)
        assert np.abs(grad - ref_grad).max() <= 1e-5 * np.abs(ref_grad).max(), (name, path)


def _ohem_cfg(thresh, min_kept, **kw):
    return dict(CFG, criterion=dict(name="OHEM", kwargs=dict(ignore_index=255, thresh=thresh, min_kept=min_kept)), **kw)


def test_ohem_step_matches_reference_fixture(dev):
    from semivl_amd.train import LOSS_NAMES, semivl_train_step
    z, c = load_fixture("tiny")
    zo = np.load(os.path.join(GOLDEN, "semivl_ohem.npz"))
    kw = eval(str(zo["criterion"]))["kwargs"]
    hip = build_hip(c)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    hip.to(dev)
    iters, total = [int(v) for v in zo["iters"]]
    cfg = _ohem_cfg(kw["thresh"], kw["min_kept"], conf_thresh=c["conf_thresh"])
    hip.train()
    losses, aux = semivl_train_step(hip, to_dev(fixture_batch(z, c), dev), iters, total, cfg,
                                    fp_masks=[m.to(dev) for m in fixture_fp_masks(z, c)], return_aux=True)
    assert np.array_equal(aux["mask_x_ohem"].cpu().numpy().astype(np.uint8), zo["mask_x_ohem"])
    losses = losses.cpu().numpy()
    for i, k in enumerate(LOSS_NAMES):
        assert abs(losses[i] - float(zo[k])) < 1e-3 * max(1.0, abs(float(zo[k]))), (k, losses[i], float(zo[k]))
    grads = {k: p.grad for k, p in hip.named_parameters() if p.grad is not None}
    assert sorted(grads) == [str(s) for s in zo["grad_names"]]
    for k, g in grads.items():
        ref = zo["gnorm/" + k]
        floor = 1e-5 if k == "decode_head.head.bias" else 1e-7
        assert abs(g.norm().item() - ref[0]) < 2e-3 * ref[0] + floor, f"grad norm of {k}: {g.norm().item()} vs {ref[0]}"
        if ("grad/" + k) in zo.files:
            full = zo["grad/" + k]
            e = np.abs(g.cpu().numpy() - full).max() / max(np.abs(full).max(), 1e-3 if k == "decode_head.head.bias" else 1e-5)
            assert e < 5e-3, f"grad of {k}: rel max err {e}"


def _step(build, batch_fn, masks, cfg, dev):
    from semivl_amd.train import semivl_train_step
    m = build()
    losses, aux = semivl_train_step(m, batch_fn(), 1, 10, cfg, fp_masks=masks, return_aux=True)
    return losses.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, aux


def _assert_equivalent(build, batch_fn, masks, cfg_ohem, cfg_ce, dev):
    """the OHEM step == the plain cross-entropy step on the OHEM step's relabelled mask_x, bit for bit"""
    l1, g1, aux = _step(build, batch_fn, masks, cfg_ohem, dev)
    rel = aux["mask_x_ohem"]
    assert rel is not None

    def relabelled():
        b = batch_fn()
        b["mask_x"] = rel.clone()
        return b
    l2, g2, aux2 = _step(build, relabelled, masks, cfg_ce, dev)
    assert aux2["mask_x_ohem"] is None
    assert torch.equal(l1, l2), (l1, l2)
    assert sorted(g1) == sorted(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    return l1, rel


@pytest.mark.parametrize("fuse", [True, False])
def test_ohem_step_equals_ce_step_on_relabelled_mask(dev, fuse):
    z, c = load_fixture("tiny")
    zo = np.load(os.path.join(GOLDEN, "semivl_ohem.npz"))
    kw = eval(str(zo["criterion"]))["kwargs"]

    def build():
        hip = build_hip(c)
        hip.load_state_dict(fixture_state(z, c, hip), strict=True)
        return hip.to(dev)
    masks = [m.to(dev) for m in fixture_fp_masks(z, c)]
    cfg_ce = dict(CFG, conf_thresh=0.05, fuse_upsample_loss=fuse)
    cfg_oh = _ohem_cfg(kw["thresh"], kw["min_kept"], conf_thresh=0.05, fuse_upsample_loss=fuse)
    _, rel = _assert_equivalent(build, lambda: to_dev(fixture_batch(z, c), dev), masks, cfg_oh, cfg_ce, dev)
    valid = int((to_dev(fixture_batch(z, c), dev)["mask_x"] != 255).sum())
    assert kw["min_kept"] < int((rel != 255).sum()) < valid


def test_fullsize_ohem_step_mode6(dev):
    """VOC 512^2, B = 2, split arithmetic (mode 6), OHEM(thresh=0.7, min_kept=200000) -- the intended generated config."""
    from semivl_amd import ops
    from semivl_amd.model.builder import build_model
    from semivl_amd.synthetic import exp40_cfg, synthetic_batch
    cfg = exp40_cfg(2, 512, 21, "pascal")
    sd = None

    def build():
        nonlocal sd
        torch.manual_seed(1234)
        m = build_model(cfg)
        if sd is None:
            sd = {k: v.clone() for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        return m.to(dev)
    batch = synthetic_batch(2, 512, 21, seed=1234, device=dev)
    cfg_ce = dict(cfg, criterion=dict(name="CELoss", kwargs=dict(ignore_index=255)))
    cfg_oh = dict(cfg, criterion=dict(name="OHEM", kwargs=dict(ignore_index=255, thresh=0.7, min_kept=200000)))
    ops.set_gemm_emulation(6)
    try:
        losses, rel = _assert_equivalent(build, lambda: {k: v.clone() for k, v in batch.items()}, None, cfg_oh, cfg_ce, dev)
    finally:
        ops.set_gemm_emulation(0)
    nv = int((batch["mask_x"] != 255).sum())
    kept = int((rel != 255).sum())
    assert kept >= min(200000, nv), (kept, nv)
    assert bool(torch.isfinite(losses).all())
