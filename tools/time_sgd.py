"""ms per VOC training step (B = 16 labeled + 16 unlabeled images, 512^2, exp-40 model and losses, split arithmetic mode 6)
with the reference's cfg-without-'optimizer' recipe -- FusedSGD.original(lr, lr_multi), semivl.py:118-121 -- against exp 40's
FusedAdamW.  usage: python tools/time_sgd.py [--steps N] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402
from semivl_amd.model.builder import build_model  # noqa: E402
from semivl_amd.synthetic import exp40_cfg, synthetic_batch  # noqa: E402
from semivl_amd.train import optimizer_from_cfg, semivl_train_step  # noqa: E402


def time_recipe(cfg, steps, warmup, dev):
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev)
    opt = optimizer_from_cfg(model, cfg)
    batch = synthetic_batch(16, 512, 21, seed=1234, device=dev)
    for i in range(warmup):
        semivl_train_step(model, batch, i, 1000, cfg, optimizer=opt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        semivl_train_step(model, batch, warmup + i, 1000, cfg, optimizer=opt)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    kind, n = type(opt).__name__, opt.total
    del model, opt
    torch.cuda.empty_cache()
    return ms, kind, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.set_gemm_emulation(6)
    adamw = exp40_cfg(16, 512, 21, "pascal")
    original = {k: v for k, v in adamw.items() if k != "optimizer"}
    original.update(lr=0.001, lr_multi=10.0)          # config_from_vars(opt='original') for pascal
    res = {}
    for name, cfg in (("FusedAdamW (exp 40)", adamw), ("FusedSGD.original", original)):
        ms, kind, n = time_recipe(cfg, a.steps, a.warmup, dev)
        res[name] = dict(ms_per_step=round(ms, 2), optimizer=kind, arena_floats=n)
        print(f"{name:22s} {kind:10s} {ms:8.1f} ms/step  {32e3 / ms:6.1f} img/s  ({n / 1e6:.1f} M floats in the arena)", flush=True)
    d = res["FusedSGD.original"]["ms_per_step"] - res["FusedAdamW (exp 40)"]["ms_per_step"]
    print(f"FusedSGD.original - FusedAdamW = {d:+.2f} ms/step")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), batch="16 + 16 x 512^2, VOC", steps=a.steps, warmup=a.warmup,
                           recipes=res), f, indent=1)


if __name__ == "__main__":
    main()
