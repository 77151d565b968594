"""ms per VOC training step (B = 16 labeled + 16 unlabeled images, 512^2, exp-40 recipe, split arithmetic mode 6, fused AdamW) of
full fine-tuning (model_args freeze_backbone=False: every backbone tensor trains) at each stochastic-depth rate of --rates, in
the same call; the first rate is timed again at the end and reported as `<rate>_again` (the spread of the same recipe).  The rate
`none` leaves the backbone dict untouched, so the tool also runs on a checkout that does not know the option: --root names the
checkout whose package is imported (default: this one).  Prints one JSON line at the end (profiles/droppath_step_times.json
holds one per checkout).
usage: python tools/time_droppath.py [--rates none,0,0.1] [--steps N] [--warmup W] [--batch B] [--root DIR]"""
import argparse
import copy
import json
import os
import sys
import time

import torch


def time_recipe(mods, rate, steps, warmup, batch_size, dev):
    build_model, load_model_cfg, exp40_cfg, synthetic_batch, FusedAdamW, semivl_train_step = mods
    cfg = exp40_cfg(batch_size, 512, 21, "pascal")
    margs = dict(cfg["model_args"], freeze_backbone=False)
    if rate is not None:
        bb = copy.deepcopy(load_model_cfg(cfg["model"].replace("mmseg.", ""))["model"]["backbone"])
        bb.update(drop_path_rate=rate)
        margs["backbone"] = bb
    cfg["model_args"] = margs
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev)
    opt = FusedAdamW(model, cfg["optimizer"])
    ntrain = sum(p.numel() for p in model.backbone._trainable())
    batch = synthetic_batch(batch_size, 512, 21, seed=1234, device=dev)
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
    ap.add_argument("--rates", default="0,0.1")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from semivl_amd import ops
    from semivl_amd.model.builder import build_model, load_model_cfg
    from semivl_amd.synthetic import exp40_cfg, synthetic_batch
    from semivl_amd.train import FusedAdamW, semivl_train_step
    mods = (build_model, load_model_cfg, exp40_cfg, synthetic_batch, FusedAdamW, semivl_train_step)
    dev = torch.device("cuda:0")
    ops.set_gemm_emulation(6)
    rates = [None if r == "none" else float(r) for r in a.rates.split(",")]
    res = {}
    for j, rate in enumerate(rates + rates[:1]):
        name = ("none" if rate is None else f"{rate:g}") + ("_again" if j == len(rates) else "")
        ms, n = time_recipe(mods, rate, a.steps, a.warmup, a.batch, dev)
        res[name] = dict(ms_per_step=round(ms, 2), trainable_backbone_params=n)
        print(f"drop_path_rate {name:10s} {ms:8.1f} ms/step  {2e3 * a.batch / ms:6.1f} img/s  trainable backbone params "
              f"{n / 1e6:.2f} M", flush=True)
    out = dict(tool="time_droppath", root=os.path.basename(os.path.abspath(a.root)), device=torch.cuda.get_device_name(0),
               batch=a.batch, crop=512, gemm_emulation=6, recipe="freeze_backbone=False", steps=a.steps, warmup=a.warmup,
               rates=res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
