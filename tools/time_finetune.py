"""ms per VOC training step (B = 16 labeled + 16 unlabeled images, 512^2, exp-40 recipe, split arithmetic mode 6, fused AdamW) with the default
`ftap` backbone (attention projections + pos_embed train) against full fine-tuning (model_args freeze_backbone=False:
every CLIP ViT tensor trains).  usage: python tools/time_finetune.py [--steps N] [--warmup W]"""
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


def time_recipe(freeze_backbone, steps, warmup, dev):
    cfg = exp40_cfg(16, 512, 21, "pascal")
    if not freeze_backbone:
        cfg["model_args"] = dict(cfg["model_args"], freeze_backbone=False)
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev)
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
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.set_gemm_emulation(6)
    res = {}
    for name, fr in (("ftap (default)", True), ("freeze_backbone=False", False)):
        ms, n = time_recipe(fr, a.steps, a.warmup, dev)
        res[name] = ms
        print(f"{name:24s} {ms:8.1f} ms/step  {32e3 / ms:6.1f} img/s  trainable backbone params {n / 1e6:.1f} M", flush=True)
    base, ft = res["ftap (default)"], res["freeze_backbone=False"]
    print(f"full fine-tuning costs {ft - base:.1f} ms/step (x{ft / base:.3f})")


if __name__ == "__main__":
    main()
