"""ms per VOC training step (B = 16 labeled + 16 unlabeled images, 512^2, exp-40 recipe, split arithmetic mode 6, fused AdamW) with the default
`ftap` backbone (attention projections + pos_embed train) against LoRA-only training (adapters of rank 4 on q, k, v, o of all
12 blocks, exclude_keys=['lora']: the CLIP ViT itself stays frozen), in the same call.
usage: python tools/time_lora.py [--steps N] [--warmup W] [--rank R]"""
import argparse
import copy
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402
from semivl_amd.model.builder import build_model, load_model_cfg  # noqa: E402
from semivl_amd.synthetic import exp40_cfg, synthetic_batch  # noqa: E402
from semivl_amd.train import FusedAdamW, semivl_train_step  # noqa: E402


def time_recipe(lora_rank, steps, warmup, dev):
    cfg = exp40_cfg(16, 512, 21, "pascal")
    if lora_rank:
        bb = copy.deepcopy(load_model_cfg(cfg["model"].replace("mmseg.", ""))["model"]["backbone"])
        bb.update(lora_layers=list(range(bb["num_layers"])), lora_r=lora_rank, lora_scaling=1.0, lora_targets="qkvo")
        cfg["model_args"] = dict(cfg["model_args"], backbone=bb, freeze_backbone=True, exclude_keys=["lora"])
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev)
    if lora_rank:     # b_* = 0 at init: give the adapters something to merge
        with torch.no_grad():
            for n, p in model.backbone.named_parameters():
                if ".lora.b_" in n:
                    p.normal_(std=0.02)
    opt = FusedAdamW(model, cfg["optimizer"])
    ntrain = sum(p.numel() for p in model.backbone.parameters() if p.requires_grad)
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
    del model, opt
    torch.cuda.empty_cache()
    return ms, ntrain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rank", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.set_gemm_emulation(6)
    res = {}
    for name, rank in (("ftap (default)", 0), (f"LoRA only (r={a.rank}, qkvo x 12)", a.rank), ("ftap (again)", 0)):
        ms, n = time_recipe(rank, a.steps, a.warmup, dev)
        res[name] = ms
        print(f"{name:28s} {ms:8.1f} ms/step  {32e3 / ms:6.1f} img/s  trainable backbone params {n / 1e6:.2f} M", flush=True)
    base = 0.5 * (res["ftap (default)"] + res["ftap (again)"])
    lo = [v for k, v in res.items() if k.startswith("LoRA")][0]
    print(f"LoRA-only costs {lo - base:+.1f} ms/step against ftap (x{lo / base:.3f})")


if __name__ == "__main__":
    main()
