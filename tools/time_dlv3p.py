"""ms per VOC training step (B = 16 labeled + 16 unlabeled images, 512^2, split arithmetic mode 6, fused AdamW) of the
DeepLabV3+ ablation model `vlm-dlv3p-bn12-sk4-ftap-mcvitb` (experiment 41) next to the VLG model of experiment 40 in the
same run.  Context, not a gate: the DeepLabV3+ head works on the 32 x 32 token map and is small next to the ViT; its step
decodes all 4 B samples (BatchNorm statistics) and takes the unfused loss path (logits resized to the crop).
usage: python tools/time_dlv3p.py [--steps N] [--warmup W]"""
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


def time_model(model_name, steps, warmup, dev):
    cfg = dict(exp40_cfg(16, 512, 21, "pascal"), model=model_name)
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
        losses = semivl_train_step(model, batch, warmup + i, 1000, cfg, optimizer=opt)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    assert bool(torch.isfinite(losses).all()), losses
    del model, opt
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.set_gemm_emulation(6)
    res = {}
    for name in ("mmseg.vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb", "mmseg.vlm-dlv3p-bn12-sk4-ftap-mcvitb"):
        res[name] = time_model(name, a.steps, a.warmup, dev)
        print(f"{name:45s} {res[name]:8.1f} ms/step  {32e3 / res[name]:6.1f} img/s", flush=True)


if __name__ == "__main__":
    main()
