"""svl_sgd_step against svl_adamw_step on one 31.4 M-float arena (the VOC model's trainable set: 121 segments), with and
without the EMA teacher, in ONE process: the variants are timed interleaved, round after round, and the median round is
reported as ms per launch, achieved bytes/s on each kernel's own byte count (SGD 20 / 28 B per parameter, AdamW 28 / 36) and
the fraction of the 8 TB/s HBM peak.  usage: python tools/bench_sgd.py [--rounds R] [--launches N] [--out FILE.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--floats", type=int, default=31_400_000)
    ap.add_argument("--nseg", type=int, default=121)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    per = a.floats // a.nseg // 4 * 4
    offs = [i * per for i in range(a.nseg)]
    total = a.floats // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    p, g, m, v, ema = (torch.randn(total, device=dev, generator=gen) * s for s in (1.0, 1e-3, 1e-3, 1e-6, 1.0))
    v.abs_()
    seg_off = torch.tensor(offs + [total], dtype=torch.int64, device=dev)
    seg_lr = torch.full((a.nseg,), 1e-6, device=dev)
    seg_wd = torch.full((a.nseg,), 1e-4, device=dev)
    variants = {
        "sgd": (20, lambda: ops.sgd_step(p, g, m, seg_off, seg_lr, seg_wd, a.nseg, 0.9, 0.0, False, 2)),
        "sgd+ema": (28, lambda: ops.sgd_step(p, g, m, seg_off, seg_lr, seg_wd, a.nseg, 0.9, 0.0, False, 2, 1.0, ema, 0.99)),
        "adamw": (28, lambda: ops.adamw_step(p, g, m, v, seg_off, seg_lr, seg_wd, a.nseg, 0.9, 0.999, 1e-8, 2)),
        "adamw+ema": (36, lambda: ops.adamw_step(p, g, m, v, seg_off, seg_lr, seg_wd, a.nseg, 0.9, 0.999, 1e-8, 2, 1.0, ema, 0.99)),
    }
    for _, fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, (_, fn) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.launches)
    res = {}
    for name, (bpp, _) in variants.items():
        ts = sorted(times[name])
        ms = ts[len(ts) // 2]
        rate = bpp * total / (ms * 1e-3)
        res[name] = dict(ms=round(ms, 4), ms_min=round(ts[0], 4), ms_max=round(ts[-1], 4), bytes_per_param=bpp,
                         bytes_per_s=round(rate), fraction_of_8TBps_peak=round(rate / PEAK, 3))
        print(f"{name:10s} {ms * 1e3:8.1f} us  ({ts[0] * 1e3:.1f} .. {ts[-1] * 1e3:.1f})  {bpp} B/param  "
              f"{rate / 1e12:5.2f} TB/s  {rate / PEAK:5.1%} of peak")
    out = dict(arena_floats=total, nseg=a.nseg, rounds=a.rounds, launches_per_round=a.launches,
               device=torch.cuda.get_device_name(0), kernels=res,
               sgd_over_adamw=round(res["sgd"]["ms"] / res["adamw"]["ms"], 4),
               sgd_ema_over_adamw_ema=round(res["sgd+ema"]["ms"] / res["adamw+ema"]["ms"], 4))
    print(f"sgd / adamw = {out['sgd_over_adamw']:.3f} (20 / 28 = {20 / 28:.3f} if both ran at one HBM rate); "
          f"with EMA {out['sgd_ema_over_adamw_ema']:.3f} (28 / 36 = {28 / 36:.3f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
