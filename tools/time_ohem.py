"""ms per VOC training step (B = 16 labeled + 16 unlabeled images, 512^2, exp-40 recipe, split arithmetic mode 6, fused
AdamW) with the supervised criterion CELoss against OHEM(thresh=0.7, min_kept=200000), and the three OHEM passes alone
(target probability on the head-resolution logits, radix-select threshold, relabel) on that step's shapes.
usage: python tools/time_ohem.py [--steps N] [--warmup W]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402
from semivl_amd.model.builder import build_model  # noqa: E402
from semivl_amd.synthetic import exp40_cfg, synthetic_batch  # noqa: E402
from semivl_amd.train import FusedAdamW, semivl_train_step  # noqa: E402


def time_recipe(criterion, steps, warmup, dev):
    cfg = dict(exp40_cfg(16, 512, 21, "pascal"), criterion=criterion)
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev)
    opt = FusedAdamW(model, cfg["optimizer"])
    batch = synthetic_batch(16, 512, 21, seed=1234, device=dev)
    for i in range(warmup):
        opt.zero_grad()
        semivl_train_step(model, batch, i, 1000, cfg, optimizer=opt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        opt.zero_grad()
        semivl_train_step(model, batch, warmup + i, 1000, cfg, optimizer=opt)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    hs = model.head_res_size((512, 512))
    del model, opt
    torch.cuda.empty_cache()
    return ms, hs


def time_kernels(hs, dev, reps=50):
    """the three passes at B = 16, 21 classes, head resolution hs -> 512^2 (us each, median of `reps` event timings)"""
    B, N, H, W = 16, 21, 512, 512
    g = torch.Generator(device=dev).manual_seed(1)
    low = torch.randn(B, N, hs[0], hs[1], device=dev, generator=g) * 3
    t = torch.randint(0, N, (B, H, W), device=dev, generator=g)
    t[torch.rand(B, H, W, device=dev, generator=g) < 0.1] = 255
    nv = ops.zeros(1, dtype=torch.int64, device=dev)
    ops.count_valid(t, nv)
    prob = ops.target_prob(low, t, up=(H, W, False))
    n = prob.numel()
    thr = ops.ohem_threshold(prob, min(n, 200000), nv, 200000, 0.7)
    out = torch.empty_like(t)
    cnt = ops.zeros(1, dtype=torch.int64, device=dev)
    from semivl_amd import lib as L
    lib = L.load()
    ws = torch.empty(lib.svl_ohem_ws_bytes(n), dtype=torch.uint8, device=dev)
    passes = {
        "target_prob_up": lambda: ops.target_prob(low, t, up=(H, W, False)),
        "threshold (radix select)": lambda: L.check(lib.svl_ohem_threshold_f32(
            ops._p(prob), n, min(n, 200000), ops._p(nv), 200000, 0.7, ops._p(ws), ops._p(thr), ops._st()), "thr"),
        "relabel": lambda: L.check(lib.svl_ohem_relabel_i64(ops._p(t), ops._p(prob), n, ops._p(thr), ops._p(out),
                                                            ops._p(cnt), ops._st()), "relabel"),
    }
    res = {}
    for name, fn in passes.items():
        for _ in range(5):
            fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        res[name] = sorted(ts)[len(ts) // 2]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.set_gemm_emulation(6)
    res = {}
    hs = None
    for name, crit in (("CELoss", dict(name="CELoss", kwargs=dict(ignore_index=255))),
                       ("OHEM(0.7, 200000)", dict(name="OHEM", kwargs=dict(ignore_index=255, thresh=0.7, min_kept=200000)))):
        ms, hs = time_recipe(crit, a.steps, a.warmup, dev)
        res[name] = ms
        print(f"{name:20s} {ms:8.1f} ms/step  {32e3 / ms:6.1f} img/s", flush=True)
    base, oh = res["CELoss"], res["OHEM(0.7, 200000)"]
    print(f"OHEM costs {oh - base:.2f} ms/step (x{oh / base:.4f})")
    for name, us in time_kernels(hs, dev).items():
        print(f"  {name:26s} {us:8.1f} us (B = 16, 512^2, head resolution {hs[0]}x{hs[1]})")


if __name__ == "__main__":
    main()
