"""GPU: the DeepLabV3+ ablation head (semivl_amd/model/dlv3p_head.py) against the reference's own modules
(tests/golden/dlv3p_head.npz, written by tests/golden/gen_golden_dlv3p.py), one training step, the sliding-window
evaluator and the two-process SyncBN exchange.

The fixture stores neither inputs nor parameters: both are closed-form functions of the flat element index (an integer
hash), restated here independently of the generator.  Results of more than FULL_MAX elements are stored as values at SUB
hashed positions plus a count sketch of SK signed bucket sums (E ||sk(a) - sk(b)||^2 = ||a - b||^2, relative standard
deviation sqrt(2 / SK) = 6 %) and the tensor's L2 norm; see the generator's docstring.

Limits: the project's north_star limits of BASELINE.json -- logits 1e-3 (absolute), per-tensor gradient relative L2 4e-3;
running statistics are held to the logits' limit.  A tensor over its limit is not given a wider one: its distance from
the fixture's float64 run is compared with the fp32 reference's own distance from that run and must stay within the 4 x
cap of tests/test_fullsize_gpu.py; the ratio is printed (-s)."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LOGIT_TOL, GRAD_TOL, FP64_CAP = 1e-3, 4e-3, 4.0
FULL_MAX, SUB, SK = 10240, 1024, 512
C1, C4, C1P, DIL = 768, 512, 48, (6, 12, 18)
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ closed-form data
def _hash32(i, salt):
    """int64 tensor of indices -> 32-bit hashes as non-negative int64 (int64 products wrap; their low 32 bits are exact)."""
    x = (i + salt * 0x9E3779B1) & M32
    x = (x * 2654435761) & M32
    x = x ^ (x >> 15)
    x = (x * 2246822519) & M32
    x = x ^ (x >> 13)
    x = (x * 3266489917) & M32
    return x ^ (x >> 16)


def _salt(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name)) % 100003


def _unit(n, name):
    return _hash32(torch.arange(n, dtype=torch.int64), _salt(name)).double() / 2.0 ** 32 * 2.0 - 1.0


def _param(name, shape):
    u = _unit(int(np.prod(shape)), name)
    if len(shape) == 4:
        v = u * float(np.sqrt(6.0 / (shape[1] * shape[2] * shape[3])))
    elif name.endswith(".weight"):
        v = 1.0 + 0.25 * u
    elif name.startswith("head.6"):
        v = 0.1 * u
    else:
        v = 0.25 * u
    return v.float().view(shape)


def _feature(name, n, HW, C):
    return (_unit(n * HW * C, name).view(n, HW, C) + _unit(n * C, name + ".offset").view(n, 1, C)).float()


def _filled_head(N, img_size, dev):
    from semivl_amd.model.dlv3p_head import DLV3PHead
    head = DLV3PHead(c1_in_channels=C1, c1_channels=C1P, dilations=DIL, img_size=img_size, in_channels=C4, in_index=3,
                     channels=256, dropout_ratio=0, num_classes=N, norm_cfg=dict(type="SyncBN", requires_grad=True),
                     align_corners=False, init_cfg=None)
    with torch.no_grad():
        for name, p in head.named_parameters():
            p.copy_(_param(name, tuple(p.shape)))
    return head.to(dev)


# ------------------------------------------------------------------------------------------------ comparison
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "dlv3p_head.npz"))


def _sketch(a, key):
    a = a.detach().double().cpu().reshape(-1)
    h = _hash32(torch.arange(a.numel(), dtype=torch.int64), _salt(key) + 2)
    sign = 1.0 - 2.0 * ((h >> 20) & 1).double()
    pos = _hash32(torch.arange(SUB, dtype=torch.int64), _salt(key) + 1) % a.numel()
    return torch.zeros(SK, dtype=torch.float64).index_add_(0, h % SK, sign * a), a[pos]


def _check(z, key, got, kind, log):
    """kind 'abs' (logits, running statistics: max |difference| <= 1e-3) or 'rel' (gradients: relative L2 <= 4e-3)."""
    got = got.detach().double().cpu()
    if key in z.files:
        ref, r64 = torch.from_numpy(z[key]).double(), torch.from_numpy(z[key + "/f64"])
        assert tuple(ref.shape) == tuple(got.shape), (key, got.shape, ref.shape)
        if kind == "abs":
            d, d_got64, d_ref64 = float((got - ref).abs().max()), float((got - r64).abs().max()), float((ref - r64).abs().max())
            lim = LOGIT_TOL
        else:
            nrm = float(r64.norm()) + 1e-30
            d, d_got64, d_ref64 = float((got - ref).norm()) / nrm, float((got - r64).norm()) / nrm, float((ref - r64).norm()) / nrm
            lim = GRAD_TOL
    else:
        assert tuple(z[key + "/shape"]) == tuple(got.shape), (key, got.shape)
        sk, sub = _sketch(got, key)
        rsk, rsk64 = torch.from_numpy(z[key + "/sk"]), torch.from_numpy(z[key + "/sk64"])
        rsub, rsub64 = torch.from_numpy(z[key + "/sub"]).double(), torch.from_numpy(z[key + "/sub64"])
        if kind == "abs":       # the stored positions element-wise, and the whole tensor's RMS difference from the sketch
            rms = float(got.numel()) ** 0.5
            d = max(float((sub - rsub).abs().max()), float((sk - rsk).norm()) / rms)
            d_got64 = max(float((sub - rsub64).abs().max()), float((sk - rsk64).norm()) / rms)
            d_ref64 = max(float((rsub - rsub64).abs().max()), float((rsk - rsk64).norm()) / rms)
            lim = LOGIT_TOL
        else:
            nrm = float(z[key + "/n2_64"]) + 1e-30
            d, d_got64, d_ref64 = float((sk - rsk).norm()) / nrm, float((sk - rsk64).norm()) / nrm, float((rsk - rsk64).norm()) / nrm
            lim = GRAD_TOL
    ratio = d_got64 / max(d_ref64, 1e-30)
    line = f"{key}: distance {d:.2e} (limit {lim:.0e}); from float64 {d_got64:.2e}, reference's own {d_ref64:.2e}, ratio {ratio:.2f}"
    log.append(line)
    if d > lim:
        print("OVER ITS LIMIT, judged against the float64 run:", line)
        assert ratio <= FP64_CAP, line
    return d


@pytest.mark.parametrize("mode", [0, 6])
@pytest.mark.parametrize("case", ["A", "B"])
def test_head_matches_reference_modules(dev, golden, case, mode):
    """Train-mode logits of both halves of the need_fp batch, the running statistics that step leaves, every parameter
    gradient and both input gradients of sum(logits * G), then the eval-mode logits read from those statistics."""
    from semivl_amd import ops
    z = golden
    N, n, H, W = (int(v) for v in z[f"{case}/dims"])
    tag = f"{N}x{n}x{H}x{W}"
    log = []
    ops.set_gemm_emulation(mode)
    try:
        head = _filled_head(N, 16 * max(H, W), dev).train()
        c1 = _feature(f"c1.{tag}", n, H * W, C1).to(dev).requires_grad_(True)
        c4 = _feature(f"c4.{tag}", n, H * W, C4).to(dev).requires_grad_(True)
        masks = [torch.from_numpy(z[f"{case}/mask/{k}"].astype(np.float32)).to(dev) for k in ("c1", "c4")]
        assert torch.equal(masks[0].cpu(), (_unit(n * C1, f"m1.{tag}") < 0).float().view(n, C1))    # the two hash restatements agree
        out = head.forward_tokens([c1, c4], None, (H, W), masks, 0.5, out_size=(H, W))
        assert tuple(out.shape) == (2 * n, N, H, W)
        G = _unit(out.numel(), f"G.{tag}").view(out.shape).float().to(dev)
        out.backward(G)
        torch.cuda.synchronize()
        _check(z, f"{case}/logits_train", out, "abs", log)
        for name, b in head.named_buffers():
            if name.endswith("num_batches_tracked"):
                assert int(b) == 1 == int(z[f"{case}/stat/{name}"]), name
            else:
                _check(z, f"{case}/stat/{name}", b, "abs", log)
        for name, p in head.named_parameters():
            assert p.grad is not None, name
            _check(z, f"{case}/grad/{name}", p.grad, "rel", log)
        _check(z, f"{case}/grad_in/c1", c1.grad, "rel", log)
        _check(z, f"{case}/grad_in/c4", c4.grad, "rel", log)
        head.eval()
        with torch.no_grad():
            ev = head.forward_tokens([c1.detach(), c4.detach()], None, (H, W), None, 0.5, out_size=(H, W))
        _check(z, f"{case}/logits_eval", ev, "abs", log)
        # the reference-signature forward (NCHW maps, resize to image_size^2) is the same decode + one bilinear resize
        maps = [t.detach().view(n, H, W, -1).permute(0, 3, 1, 2) for t in (c1, c4)]
        with torch.no_grad():
            pm = head([[maps, None], None, None], force_output_pred_masks=True)["pred_masks"]
        S_ = head.image_size
        assert tuple(pm.shape) == (n, N, S_, S_)
        assert torch.equal(pm, ops.bilinear_planes_fwd(ev.contiguous(), H, W, False, S_, S_))
    finally:
        ops.set_gemm_emulation(0)
    print(f"\n[dlv3p case {case} mode {mode}]\n  " + "\n  ".join(log))


# ------------------------------------------------------------------------------------------------ training step / evaluator
STEP_CFG = dict(conf_thresh=0.05, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
                maskclip_consistency_lambda=[0.1, 0])


def _tiny_model(tmp_path, monkeypatch, dev, crop=64, nclass=5):
    """The ftap row of experiment 41 at crop 64 with 5 classes: build_model resolves the text embeddings relative to the
    working directory first, so a 5-class embedding file there stands in for the 21-class one of the package."""
    from semivl_amd.model.builder import build_model
    rows = json.load(open(os.path.join(HERE, "golden", "experiment41_cfgs.json")))
    row = next(c for c in rows.values() if c["model"] == "mmseg.vlm-dlv3p-bn12-sk4-ftap-mcvitb")
    d = tmp_path / "configs" / "_base_" / "datasets" / "text_embedding"
    d.mkdir(parents=True)
    t = torch.randn(nclass, 512, generator=torch.Generator().manual_seed(5))
    np.save(d / "voc12_wbg_single.npy", (t / t.norm(dim=1, keepdim=True)).numpy().astype(np.float16))
    monkeypatch.chdir(tmp_path)
    cfg = dict(row, crop_size=crop, nclass=nclass, clip_encoder="mcvit16", allow_random_init=True)
    torch.manual_seed(11)
    return build_model(cfg).to(dev), cfg


def test_train_step(dev, tmp_path, monkeypatch):
    from semivl_amd.optim import optimizer_from_cfg
    from semivl_amd.synthetic import synthetic_batch
    from semivl_amd.train import semivl_train_step
    B, S_, N = 2, 64, 5
    model, cfg = _tiny_model(tmp_path, monkeypatch, dev, S_, N)
    assert model.head_res_size((S_, S_)) is None
    state = {k: v.clone() for k, v in model.state_dict().items()}
    fp_masks = [(torch.rand(2 * B, c, generator=torch.Generator().manual_seed(7 + c)) < 0.5).float().to(dev) for c in (C1, C4)]
    results = []
    for _ in range(2):
        model.load_state_dict(state)
        for p in model.parameters():
            p.grad = None
        batch = synthetic_batch(B, S_, N, seed=99, device=dev)
        losses = semivl_train_step(model, batch, 1, 10, STEP_CFG, fp_masks=[m.clone() for m in fp_masks])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(losses).all()), losses
        grads = {}
        for n_, p in model.named_parameters():
            if n_.startswith("clip_encoder."):
                continue
            if p.requires_grad:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n_
                if n_.startswith("decode_head."):
                    assert float(p.grad.abs().max()) > 0, n_
                grads[n_] = p.grad.clone()
            else:
                assert p.grad is None, n_
        bufs = {n_: b.clone() for n_, b in model.decode_head.named_buffers()}
        for n_, b in bufs.items():      # the [w, x, w_fp, x_fp] forward and the [s1, s2] forward: two updates per step
            if n_.endswith("num_batches_tracked"):
                assert int(b) == 2, (n_, int(b))
            elif n_.endswith("running_mean"):
                assert float(b.abs().max()) > 0, n_
        results.append((losses.clone(), grads, bufs))
    (l0, g0, b0), (l1, g1, b1) = results
    assert torch.equal(l0, l1)
    for n_ in g0:
        assert torch.equal(g0[n_], g1[n_]), n_
    for n_ in b0:
        assert torch.equal(b0[n_], b1[n_]), n_
    # the optimizer the experiment dict builds sees the head's tensors: 'head' -> lr x 10 for every decode_head tensor
    model.load_state_dict(state)
    opt = optimizer_from_cfg(model, cfg)
    lr = {g_["name"]: g_["lr"] for g_ in opt.groups}
    base = cfg["optimizer"]["lr"]
    heads = [n_ for n_ in lr if n_.startswith("decode_head.head.")]
    assert len(heads) == 8 and all(lr[n_] == pytest.approx(10 * base) for n_ in heads)
    before = model.decode_head.head[6].weight.detach().clone()
    losses = semivl_train_step(model, synthetic_batch(B, S_, N, seed=99, device=dev), 1, 10, STEP_CFG, optimizer=opt,
                               fp_masks=[m.clone() for m in fp_masks])
    torch.cuda.synchronize()
    assert torch.equal(losses, l0) and not torch.equal(model.decode_head.head[6].weight.detach(), before)


def test_sliding_window_predict(dev, tmp_path, monkeypatch):
    from semivl_amd.evaluate import predict
    model, cfg = _tiny_model(tmp_path, monkeypatch, dev, 64, 5)
    model.eval()
    img = torch.randn(1, 3, 96, 80, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        pred = predict(model, img, torch.zeros(1, 96, 80, dtype=torch.int64, device=dev), "sliding_window",
                       dict(crop_size=64, nclass=5))
    assert tuple(pred.shape) == (1, 96, 80) and pred.dtype == torch.int64
    assert int(pred.min()) >= 0 and int(pred.max()) < 5


# ------------------------------------------------------------------------------------------------ SyncBN, two processes
def _sync_inputs(n, H, W):
    return _feature("sync.c1", n, H * W, C1), _feature("sync.c4", n, H * W, C4), _unit(n * 5 * H * W, "sync.G").float().view(n, 5, H, W)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    n, H, W = 4, 6, 5
    c1, c4, G = _sync_inputs(n, H, W)
    half = n // world
    sl = slice(rank * half, (rank + 1) * half)
    head = _filled_head(5, 96, dev).train()
    a, b = c1[sl].to(dev).requires_grad_(True), c4[sl].to(dev).requires_grad_(True)
    out = head.forward_tokens([a, b], None, (H, W), None, 0.5, out_size=(H, W))
    out.backward(G[sl].to(dev))
    torch.cuda.synchronize()
    q.put((rank, out.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in head.named_parameters()},
           {k: v.cpu().numpy() for k, v in head.named_buffers()}, a.grad.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_syncbn_two_ranks_equal_one_big_batch(dev):
    """Two gloo processes on the one GPU, each decoding half of a batch: logits, running statistics and the rank-summed
    parameter gradients equal a single-process decode of the whole batch (the limits of the side encoder's SyncBN test in
    tests/test_multiproc_gpu.py)."""
    n, H, W = 4, 6, 5
    c1, c4, G = _sync_inputs(n, H, W)
    ref = _filled_head(5, 96, dev).train()
    a = c1.to(dev).requires_grad_(True)
    out = ref.forward_tokens([a, c4.to(dev)], None, (H, W), None, 0.5, out_size=(H, W))
    out.backward(G.to(dev))
    torch.cuda.synchronize()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29950 + os.getpid() % 40
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    got = np.concatenate([r[1] for r in res], 0)
    assert np.abs(got - out.detach().cpu().numpy()).max() < 2e-4
    for k, b in ref.named_buffers():
        for r in res:
            assert np.abs(r[3][k].astype(np.float64) - b.cpu().numpy()).max() < 1e-4 * max(1.0, float(b.abs().max())), k
    for k, p in ref.named_parameters():
        g = sum(r[2][k] for r in res)
        e = np.linalg.norm(g - p.grad.cpu().numpy()) / (np.linalg.norm(p.grad.cpu().numpy()) + 1e-12)
        assert e < 3e-2, (k, e)
    gin = np.concatenate([r[4] for r in res], 0)
    e = np.linalg.norm(gin - a.grad.cpu().numpy()) / np.linalg.norm(a.grad.cpu().numpy())
    assert e < 3e-2, e
