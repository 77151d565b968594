"""Gradient-norm clipping on the real arenas: the VOC `ftap` model (31.4 M floats) and full fine-tuning
(model_args freeze_backbone=False, 89.0 M floats), each with its own segment table.  Three measurements, written to
profiles/gradclip_times.json:

  norm     svl_grad_clip_f32 alone (both launches), L2 and max norm, as warmed launches in alternating rounds between device
           events (tools/bench_sgd.py's scheme).  `warm`: the same arena again and again -- the 126 MB arena then lies in the
           256 MiB Infinity Cache, as it largely does in a training step, where backward has just written it; `cold`: the
           launches rotate over copies that together exceed the cache twice, so every read comes from HBM.  Bytes: 4 per
           parameter, read once.
  step     svl_sgd_step / svl_adamw_step with the host-float scale and their *_dscale forms on the same buffers.
  recipe   ms per step of the VOC B = 16 mode-6 full fine-tuning recipe with and without grad_clip=dict(max_norm=1.0) on ONE
           model and optimizer (set_grad_clip between rounds), alternating.

usage: python tools/time_gradclip.py [--rounds R] [--launches N] [--steps K] [--warmup W] [--out FILE.json] [--skip-recipe]"""
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
from semivl_amd.train import FusedAdamW, semivl_train_step  # noqa: E402

PEAK = 8.0e12
CACHE_BYTES = 256 * 2 ** 20


def build(full, dev):
    cfg = exp40_cfg(16, 512, 21, "pascal")
    if full:
        cfg["model_args"] = dict(cfg["model_args"], freeze_backbone=False)
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev)
    return cfg, model, FusedAdamW(model, cfg["optimizer"])


def rounds_of(variants, rounds, launches):
    """{name: sorted ms per launch over the rounds}; the variants alternate inside every round."""
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / launches)
    return {k: sorted(v) for k, v in times.items()}


def summary(ts, nbytes):
    ms = ts[len(ts) // 2]
    rate = nbytes / (ms * 1e-3)
    return dict(us=round(ms * 1e3, 2), us_min=round(ts[0] * 1e3, 2), us_max=round(ts[-1] * 1e3, 2),
                bytes_per_s=round(rate), fraction_of_8TBps_peak=round(rate / PEAK, 3))


def bench_kernels(opt, rounds, launches, dev):
    """The norm pass and the step kernels on buffers of this optimizer's layout (its seg_off / seg_lr / seg_wd)."""
    total, nseg = opt.total, len(opt.groups)
    gen = torch.Generator(device=dev).manual_seed(0)
    copies = max(2, -(-2 * CACHE_BYTES // (4 * total)) + 1)       # together more than twice the Infinity Cache
    gs = [torch.randn(total, device=dev, generator=gen) * 1e-3 for _ in range(copies)]
    stats, ws = ops.zeros(4, device=dev), ops.grad_clip_ws(gs[0])
    turn = [0]

    def cold(norm_type):
        def fn():
            turn[0] = (turn[0] + 1) % copies
            ops.grad_clip(gs[turn[0]], 1.0, norm_type, stats=stats, ws=ws)
        return fn
    norm = rounds_of({"l2 warm": lambda: ops.grad_clip(gs[0], 1.0, 2.0, stats=stats, ws=ws),
                      "l2 cold": cold(2.0),
                      "max warm": lambda: ops.grad_clip(gs[0], 1.0, "inf", stats=stats, ws=ws),
                      "max cold": cold("inf")}, rounds, launches)
    out = dict(arena_floats=total, nseg=nseg, copies_rotated_when_cold=copies,
               norm={k: summary(v, 4 * total) for k, v in norm.items()})
    for k, v in out["norm"].items():
        print(f"  grad_clip {k:9s} {v['us']:8.1f} us ({v['us_min']:.1f} .. {v['us_max']:.1f})  "
              f"{v['bytes_per_s'] / 1e12:5.2f} TB/s", flush=True)
    g = gs[0]
    del gs[1:]
    p, m, v, ema = (torch.randn(total, device=dev, generator=gen) * s for s in (1.0, 1e-3, 1e-6, 1.0))
    v.abs_()
    lr = torch.full((nseg,), 1e-6, device=dev)
    sdev = torch.ones(1, device=dev)
    tabs = (opt.seg_off, lr, opt.seg_wd, nseg)
    step = rounds_of({
        "sgd": lambda: ops.sgd_step(p, g, m, *tabs, 0.9, 0.0, False, 2),
        "sgd dscale": lambda: ops.sgd_step(p, g, m, *tabs, 0.9, 0.0, False, 2, gscale_dev=sdev),
        "adamw": lambda: ops.adamw_step(p, g, m, v, *tabs, 0.9, 0.999, 1e-8, 2),
        "adamw dscale": lambda: ops.adamw_step(p, g, m, v, *tabs, 0.9, 0.999, 1e-8, 2, gscale_dev=sdev),
        "adamw+ema": lambda: ops.adamw_step(p, g, m, v, *tabs, 0.9, 0.999, 1e-8, 2, 1.0, ema, 0.99),
        "adamw+ema dscale": lambda: ops.adamw_step(p, g, m, v, *tabs, 0.9, 0.999, 1e-8, 2, ema=ema, ema_decay=0.99,
                                                   gscale_dev=sdev)}, rounds, launches)
    bpp = {"sgd": 20, "adamw": 28, "adamw+ema": 36}
    out["step"] = {k: summary(t, bpp[k.replace(" dscale", "")] * total) for k, t in step.items()}
    for k, t in out["step"].items():
        print(f"  {k:18s} {t['us']:8.1f} us ({t['us_min']:.1f} .. {t['us_max']:.1f})  {t['bytes_per_s'] / 1e12:5.2f} TB/s",
              flush=True)
    return out


def time_recipe(cfg, model, opt, steps, warmup, rounds, dev):
    batch = synthetic_batch(16, 512, 21, seed=1234, device=dev)
    it = 0
    for _ in range(warmup):
        semivl_train_step(model, batch, it, 1000, cfg, optimizer=opt)
        it += 1
    res = {"no clip": [], "grad_clip max_norm=1.0": []}
    for _ in range(rounds):
        for name in res:
            opt.set_grad_clip(None if name == "no clip" else 1.0)
            semivl_train_step(model, batch, it, 1000, cfg, optimizer=opt)      # the first step after the switch is not timed
            it += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                semivl_train_step(model, batch, it, 1000, cfg, optimizer=opt)
                it += 1
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / steps * 1e3)
    stats = [round(float(x), 6) for x in opt.grad_stats.cpu()]
    out = {k: dict(ms_per_step=round(sorted(v)[len(v) // 2], 2), rounds=[round(x, 2) for x in v]) for k, v in res.items()}
    out["last grad_stats {norm, coef, scale, nonfinite}"] = stats
    for k, v in res.items():
        print(f"  {k:24s} {sorted(v)[len(v) // 2]:8.2f} ms/step  rounds {[round(x, 2) for x in v]}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-recipe", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "gradclip_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.set_gemm_emulation(6)
    out = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, launches_per_round=a.launches, arenas={})
    for name, full in (("VOC ftap", False), ("VOC freeze_backbone=False", True)):
        cfg, model, opt = build(full, dev)
        print(f"{name}: {opt.total / 1e6:.1f} M floats, {len(opt.groups)} segments", flush=True)
        out["arenas"][name] = bench_kernels(opt, a.rounds, a.launches, dev)
        torch.cuda.empty_cache()
        if full and not a.skip_recipe:
            out["recipe"] = dict(batch="16 + 16 x 512^2, VOC, freeze_backbone=False, mode 6, FusedAdamW", steps=a.steps,
                                 warmup=a.warmup, rounds=a.step_rounds,
                                 **time_recipe(cfg, model, opt, a.steps, a.warmup, a.step_rounds, dev))
        del model, opt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
