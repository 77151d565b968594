"""ms per VOC training step (B = 16 labeled + 16 unlabeled images, 512^2, exp-40 recipe, split arithmetic mode 6, fused AdamW) of
(a) the default `ftap` backbone (attention projections + pos_embed train), (b) prompts only (num_prompt_tokens=P,
exclude_keys=['prompt']: the blocks stay frozen and launch no weight-gradient work) and (c) prompts next to the ftap tensors
(exclude_keys=['attn', 'pos_embed', 'prompt']), in the same call; (a) is timed before and after the other two and the
yardstick is the mean of the two.  Prints one JSON line at the end (profiles/prompt_step_times.json).
usage: python tools/time_prompt.py [--steps N] [--warmup W] [--prompts P] [--batch B]"""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402
from semivl_amd.model.builder import build_model, load_model_cfg  # noqa: E402
from semivl_amd.synthetic import exp40_cfg, synthetic_batch  # noqa: E402
from semivl_amd.train import FusedAdamW, semivl_train_step  # noqa: E402


def time_recipe(prompts, exclude_keys, steps, warmup, batch_size, dev):
    cfg = exp40_cfg(batch_size, 512, 21, "pascal")
    if prompts:
        bb = copy.deepcopy(load_model_cfg(cfg["model"].replace("mmseg.", ""))["model"]["backbone"])
        bb.update(num_prompt_tokens=prompts)
        cfg["model_args"] = dict(cfg["model_args"], backbone=bb, freeze_backbone=True, exclude_keys=exclude_keys)
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prompts", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.set_gemm_emulation(6)
    ftap = ["attn", "pos_embed"]
    recipes = (("ftap", 0, None), ("prompts_only", a.prompts, ["prompt"]), ("prompts_and_ftap", a.prompts, ftap + ["prompt"]),
               ("ftap_again", 0, None))
    res = {}
    for name, prompts, keys in recipes:
        ms, n = time_recipe(prompts, keys, a.steps, a.warmup, a.batch, dev)
        res[name] = dict(ms_per_step=round(ms, 2), trainable_backbone_params=n)
        print(f"{name:18s} {ms:8.1f} ms/step  {2e3 * a.batch / ms:6.1f} img/s  trainable backbone params {n / 1e6:.2f} M", flush=True)
    base = 0.5 * (res["ftap"]["ms_per_step"] + res["ftap_again"]["ms_per_step"])
    out = dict(tool="time_prompt", device=torch.cuda.get_device_name(0), batch=a.batch, crop=512, gemm_emulation=6,
               prompts=a.prompts, steps=a.steps, warmup=a.warmup, recipes=res, ftap_mean_ms=round(base, 2),
               prompts_only_over_ftap=round(res["prompts_only"]["ms_per_step"] / base, 4),
               prompts_and_ftap_over_ftap=round(res["prompts_and_ftap"]["ms_per_step"] / base, 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
