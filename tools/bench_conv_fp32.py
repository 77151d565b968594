"""Tiled 3x3 convolutions of the Up blocks in mode 0 (the exact fp32 kernel, conv3x3_tiled_kernel): forward of the four shapes
of bench_conv_planes.py, plain and with the ReLU epilogue, HIP-event timed (ms, mean of 10 calls after 3)."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
from semivl_amd import ops, lib as L

dev = torch.device("cuda:0")
ops.set_gemm_emulation(0)


def timeit(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


imgs = int(os.environ.get("IMGS", 300))
for (C, Co, Hh) in [(128, 64, 64), (64, 64, 64), (64, 32, 128), (32, 32, 128)]:
    x = torch.randn(imgs * Hh * Hh, C, device=dev)
    w = torch.randn(Co, C, 3, 3, device=dev) * 0.1
    wf, _ = ops.pack_conv_w(w)
    out = torch.zeros(imgs * Hh * Hh, Co, device=dev)
    t = timeit(lambda: ops.conv_fwd(x, C, imgs, Hh, Hh, C, wf, Co, 3, 3, 1, 1))
    print(f"fp32 fwd {C}->{Co} {Hh}x{Hh}: {t:.3f} ms path {L.load().svl_last_gemm_path()}", flush=True)
    t = timeit(lambda: ops.conv_fwd(x, C, imgs, Hh, Hh, C, wf, Co, 3, 3, 1, 1, out=out, ldo=Co, act=ops.ACT_RELU))
    print(f"fp32 fwd+relu {C}->{Co} {Hh}x{Hh}: {t:.3f} ms", flush=True)
