"""Multi-process checks on the GPU box (two gloo processes sharing its one GPU).  (1) SyncBN exchange of the Cityscapes
side encoder across data-parallel ranks: the two processes each push half of a batch through ResNetV1c; outputs, running statistics and the rank-summed parameter
gradients must equal a single-process run on the whole batch (= what torch.nn.SyncBatchNorm guarantees).  (2) One full
training step through GradAllReducer + FusedAdamW on two ranks with different data shards (gloo on the one GPU; RCCL
when the box has two)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, sd, img, dy, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from semivl_amd.model.resnet import ResNetV1c
    dev = torch.device("cuda:0")
    m = ResNetV1c()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dev).train()
    half = img.shape[0] // world
    x = torch.from_numpy(img[rank * half:(rank + 1) * half]).to(dev)
    tok, (H, W) = m.forward_tokens(x)
    tok.backward(torch.from_numpy(dy[rank * half:(rank + 1) * half]).to(dev))
    torch.cuda.synchronize()
    q.put((rank, tok.detach().cpu().numpy(), {n: p.grad.cpu().numpy() for n, p in m.named_parameters()},
           {n: b.cpu().numpy() for n, b in m.named_buffers()}))
    dist.barrier()
    dist.destroy_process_group()


def test_syncbn_two_ranks_equal_one_big_batch(dev):
    from semivl_amd.model.resnet import ResNetV1c
    torch.manual_seed(3)
    ref = ResNetV1c()
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1:
                p.copy_(1.0 + 0.2 * torch.randn_like(p) if n.endswith("weight") else 0.1 * torch.randn_like(p))
    sd = {k: v.numpy().copy() for k, v in ref.state_dict().items()}
    B, S = 4, 48
    img = torch.randn(B, 3, S, S).numpy()
    ref = ref.to(dev).train()
    tok, (H, W) = ref.forward_tokens(torch.from_numpy(img).to(dev))
    dy = torch.randn(B, H * W, 256).numpy()
    tok.backward(torch.from_numpy(dy).to(dev))
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + os.getpid() % 300
    procs = [ctx.Process(target=_worker, args=(r, world, port, sd, img, dy, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    out = np.concatenate([r[1] for r in res], 0)
    assert np.abs(out - tok.detach().cpu().numpy()).max() < 2e-4
    for n, b in ref.named_buffers():
        for r in res:
            assert np.abs(r[3][n].astype(np.float64) - b.cpu().numpy()).max() < 1e-4 * max(1.0, float(b.abs().max())), n
    for n, p in ref.named_parameters():
        g = sum(r[2][n] for r in res)                     # DDP SUM (the 1/W is folded into the optimizer)
        e = np.linalg.norm(g - p.grad.cpu().numpy()) / (np.linalg.norm(p.grad.cpu().numpy()) + 1e-12)
        assert e < 3e-2, (n, e)                           # ReLU sign flips at rounding distance, see test_model_gpu


STEP_CFG = dict(conf_thresh=0.05, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
                maskclip_consistency_lambda=[0.1, 0])


def _step_worker(rank, world, port, name, backend, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank,) + _one_step(dev, name, shards=[rank], world=world))
    dist.barrier()
    dist.destroy_process_group()


def _shard(c, rank):
    """Rank `rank`'s slice of the step inputs: DIFFERENT data on every rank (seed 500 + rank)."""
    from semivl_amd.synthetic import synthetic_batch
    return synthetic_batch(c["B"], c["S"], 21, seed=500 + rank)


def _one_step(dev, name, shards, world):
    """world > 1: this process is ONE rank, runs shard[0] and all-reduces.  world == 1: the single-process statement of
    what data parallelism must compute -- every shard's backward (each with its OWN loss normalisers)
    accumulated into one gradient arena, then one AdamW step on the mean (grad_scale = 1/len(shards))."""
    from golden_util import build_hip, fixture_fp_masks, fixture_state, load_fixture
    from semivl_amd.synthetic import exp40_cfg
    from semivl_amd.train import FusedAdamW, GradAllReducer, semivl_train_step
    z, c = load_fixture(name)
    hip = build_hip(c)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    hip.to(dev)
    opt = FusedAdamW(hip, exp40_cfg()["optimizer"])
    masks = [m.to(dev) for m in fixture_fp_masks(z, c)]
    cfg = dict(STEP_CFG, conf_mode=c.get("conf_mode", "pixelwise"))
    early = 0
    if world > 1:
        red = GradAllReducer(opt, bucket_mb=0.05, overlap=True)     # several buckets even for this tiny model
        red.broadcast_params()
        batch = {k: v.to(dev) for k, v in _shard(c, shards[0]).items()}
        semivl_train_step(hip, batch, 3, 50, cfg, optimizer=opt, reducer=red, fp_masks=masks)
        early = red.early_fires
    else:
        opt.zero_grad()
        for r in shards:
            batch = {k: v.to(dev) for k, v in _shard(c, r).items()}
            semivl_train_step(hip, batch, 3, 50, cfg, fp_masks=masks)          # accumulates into the arena
        opt.grad_scale = 1.0 / len(shards)
        opt.step()
    torch.cuda.synchronize()
    return opt.g.cpu().numpy(), opt.p.cpu().numpy(), early


def _run_two_ranks(name, backend):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + os.getpid() % 90
    procs = [ctx.Process(target=_step_worker, args=(r, world, port, name, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return res


def _check_two_ranks(dev, name, backend):
    g1, p1, _ = _one_step(dev, name, shards=[0, 1], world=1)
    res = _run_two_ranks(name, backend)
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2]), "ranks diverged"
    assert res[0][3] > 0, "no bucket was launched from inside backward"
    g2, p2 = res[0][1], res[0][2]
    # a broken / missing reduce leaves each rank with its own shard's gradient: the shards differ by O(1) relative
    own = _one_step(dev, name, shards=[0], world=1)[0]
    assert np.abs(own - g1).max() > 1e-2 * np.abs(g1).max(), "shards too similar for this test to mean anything"
    assert np.abs(g2 - g1).max() < 1e-5 * np.abs(g1).max() + 1e-9, np.abs(g2 - g1).max()
    # parameters after AdamW on the mean gradient (first step: |update| = lr per element, sign flips where the gradient is
    # rounding noise -> bound by 2 lr with lr <= 1e-3 for the decoder group)
    assert np.abs(p2 - p1).max() < 2.1e-3
    assert np.mean(np.abs(p2 - p1) > 1e-6) < 1e-3


@pytest.mark.parametrize("name", ["tiny", "offsize"])
def test_two_rank_step_different_shards_equals_accumulated_single_process(dev, name):
    """GradAllReducer (buckets launched from inside backward, SUM) + grad_scale 1/W inside FusedAdamW, two gloo ranks
    with DIFFERENT shards == one process that accumulates both shards' gradients (per-rank loss normalisers).  'offsize'
    runs an off-grid crop: pos_embed's gradient arrives through torch autograd (bicubic resize) and must be folded into
    the arena BEFORE the all-reduce."""
    _check_two_ranks(dev, name, "gloo")


def _rccl1_worker(port, name, q):
    """ONE rank, backend 'nccl' (RCCL): the real ProcessGroupNCCL code path of GradAllReducer on a one-GPU box.  The
    reducer is told `world=2` so that its multi-rank branch runs (communication stream picked against the step's
    streams, buckets fired from inside backward, stream-ordered join); a one-rank all-reduce is the identity, so with
    grad_scale reset to 1 the step must equal the reducer-less step bit for bit."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    # (the settings every rank of a multi-GPU run gets -- bench.py / semivl_amd.multi_rank_defaults: eight hardware queues,
    # no weight-gradient stream; set before the HIP runtime initialises in this spawned process)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0",
                      GPU_MAX_HW_QUEUES="8", SVL_NO_WGRAD_STREAM="1")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    from golden_util import build_hip, fixture_fp_masks, fixture_state, load_fixture
    from semivl_amd.synthetic import exp40_cfg
    from semivl_amd.train import FusedAdamW, GradAllReducer, semivl_train_step
    z, c = load_fixture(name)
    out = {}
    for tag in ("plain", "rccl"):
        hip = build_hip(c)
        hip.load_state_dict(fixture_state(z, c, hip), strict=True)
        hip.to(dev)
        opt = FusedAdamW(hip, exp40_cfg()["optimizer"])
        masks = [m.to(dev) for m in fixture_fp_masks(z, c)]
        batch = {k: v.to(dev) for k, v in _shard(c, 0).items()}
        red = None
        if tag == "rccl":
            red = GradAllReducer(opt, bucket_mb=0.05, overlap=True, world=2, profile=True)
            opt.grad_scale = 1.0            # (the one-rank SUM is the identity)
            seen = []
            real = dist.all_reduce

            def spy(t, *a, **kw):           # which stream is current when the collective is enqueued, and in which form
                seen.append((torch.cuda.current_stream().cuda_stream, kw.get("async_op", False), t.numel()))
                return real(t, *a, **kw)
            dist.all_reduce = spy
        try:
            for it in range(2):
                semivl_train_step(hip, batch, 3 + it, 50, dict(STEP_CFG), optimizer=opt, reducer=red, fp_masks=masks)
        finally:
            if tag == "rccl":
                dist.all_reduce = real
        torch.cuda.synchronize()
        out[tag] = opt.p.cpu().numpy()
        if red is not None:
            out["report"] = red.timing_report()
            out["seen"] = seen
            out["comm"] = red._comm.cuda_stream
            out["main"] = torch.cuda.current_stream().cuda_stream
            out["on_comm"] = red.on_comm_stream
            out["early"] = red.early_fires
            out["nb"] = len(red.buckets)
            out["backend"] = dist.get_backend()
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def test_one_rank_rccl_runs_the_real_process_group_on_the_communication_stream(dev):
    """The ProcessGroupNCCL branch of GradAllReducer on ONE GPU (a one-rank RCCL communicator): every bucket's
    all-reduce is enqueued with the communication stream current and in the blocking-style form that torch >= 2.8 runs ON
    that stream (not on the process group's internal one), buckets are launched from inside backward, the per-bucket HIP
    events bracket real RCCL launches (> 0 ms), the picked stream shares a hardware queue with none of the step's streams,
    and the step equals the reducer-less step bit for bit."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + os.getpid() % 200
    p = ctx.Process(target=_rccl1_worker, args=(port, "tiny", q))
    p.start()
    out = q.get(timeout=600)
    p.join(120)
    assert p.exitcode == 0
    assert out["backend"] == "nccl" and out["on_comm"], "torch >= 2.8 expected on this image"
    assert np.array_equal(out["plain"], out["rccl"]), "identity all-reduce on the communication stream changed the step"
    assert len(out["seen"]) == 2 * out["nb"] and out["nb"] >= 4
    assert all(st == out["comm"] and st != out["main"] and not asy for st, asy, _ in out["seen"])
    assert out["early"] >= out["nb"], "buckets must be launched from inside backward"
    rep = out["report"]
    assert rep and len(rep["buckets"]) == out["nb"] and all(b["ms"] > 0.0 for b in rep["buckets"]), rep
    assert rep["queues"]["comm_stream_shares_queue"] is False and "communication stream" in rep["queues"]["collective_runs_on"], rep["queues"]
    print("one-rank RCCL report:", rep)


def test_two_rank_step_rccl(dev):
    """The same check over RCCL (backend 'nccl') with the collectives on the communication stream; needs two GPUs."""
    if torch.cuda.device_count() < 2:
        pytest.skip("RCCL needs one GPU per rank; this box has %d" % torch.cuda.device_count())
    _check_two_ranks(dev, "tiny", "nccl")


def test_collective_kernels_own_their_queue_and_run_under_backward(dev):
    """Evidence that does not rest on a no-op (a world-1 RCCL all-reduce launches nothing): three training steps with
    GradAllReducer's stream-ordered branch live and an injected collective that launches REAL kernels on the communication
    stream -- a bucket-sized copy + the x2 of "SUM over two identical ranks" -- traced by rocprofv3 (tools/comm_overlap_*).
    From the trace: those kernels sit on a hardware queue none of the step's other kernels use, and > 80 % of their time
    other kernels of the step (the backward below the bucket's parameters) are running.  The reference's DDP reducer fires
    its buckets from autograd hooks inside loss.backward() (semivl.py:139-140,327): this is that overlap, observed."""
    import shutil
    import subprocess
    if shutil.which("rocprofv3") is None:
        pytest.skip("rocprofv3 not on PATH")
    env = dict(os.environ, TAG="test", GRAFT_REPO_ROOT=ROOT, SVL_COMM_B="4")
    # eight hardware queues, the setting of every rank of a multi-GPU run, also where the caller's environment sets fewer
    env["GPU_MAX_HW_QUEUES"] = "8"
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "comm_overlap_trace.sh")], env=env, capture_output=True, text=True,
                       timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "RESULT: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
