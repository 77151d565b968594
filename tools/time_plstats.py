"""The pseudo-label meter's kernel and its cost in a training step, written to profiles/plstats_times.json:

  kernel   svl_pl_stats_i64 alone at the VOC (16 x 512^2, N = 21) and ADE (N = 150) batch, 20 confidence bins, as warmed
           launches in alternating rounds between device events.  Label maps: `random` (every pixel its own class: many
           classes per wave, no contention), `blocks` (piecewise constant, 32 x 32 cells: what a segmentation map looks like)
           and `single` (one class everywhere: every lane of every wave on the same counters).  With all five maps (36 B per
           pixel) and without mc / gt (20 B).  `cold`: the launches rotate over copies of the inputs that together exceed the
           256 MiB Infinity Cache twice, so every read comes from HBM; `warm`: the same 151 MB again and again.
  step     ms per step of the VOC B = 16 mode-6 recipe with and without a PseudoLabelMeter (and a random `mask_u`) on ONE
           model and optimizer, alternating.

usage: python tools/time_plstats.py [--rounds R] [--launches N] [--steps K] [--warmup W] [--out FILE.json] [--skip-step]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402

PEAK = 8.0e12
CACHE_BYTES = 256 * 2 ** 20
B, S, BINS = 16, 512, 20


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
    return dict(us=round(ms * 1e3, 2), us_min=round(ts[0] * 1e3, 2), us_max=round(ts[-1] * 1e3, 2), bytes=nbytes,
                bytes_per_s=round(rate), fraction_of_8TBps_peak=round(rate / PEAK, 3))


def label_maps(layout, N, dev, gen):
    """(mask_w, conf, ign, mc, gt) of one batch: the pseudo-label agrees with the annotation on ~70 % of the pixels."""
    if layout == "random":
        gt = torch.randint(0, N, (B, S, S), device=dev, generator=gen)
    elif layout == "blocks":
        gt = torch.randint(0, N, (B, S // 32, S // 32), device=dev, generator=gen).repeat_interleave(32, 1).repeat_interleave(32, 2)
    else:
        gt = torch.full((B, S, S), N // 2, dtype=torch.int64, device=dev)
    r = lambda: torch.rand(B, S, S, device=dev, generator=gen)
    if layout == "single":
        p, mc, conf = gt.clone(), gt.clone(), torch.full((B, S, S), 0.97, device=dev)
    else:
        other = torch.randint(0, N, (B, S // 32, S // 32), device=dev, generator=gen).repeat_interleave(32, 1).repeat_interleave(32, 2)
        p = torch.where(r() < 0.7, gt, other if layout == "blocks" else torch.randint(0, N, (B, S, S), device=dev, generator=gen))
        mc = torch.where(r() < 0.5, gt, torch.full_like(gt, 255))
        conf = r() ** 0.25
    ign = torch.zeros(B, S, S, dtype=torch.int64, device=dev)
    ign[:, -40:, :] = 255
    return tuple(t_.contiguous() for t_ in (p, conf, ign, mc, gt))


def bench_kernel(N, rounds, launches, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    n = B * S * S
    copies = -(-2 * CACHE_BYTES // (36 * n)) + 1
    stats = ops.zeros(ops.pl_stats_len(N, BINS), dtype=torch.int64, device=dev)
    variants, nbytes = {}, {}

    def launch(sets, full):
        turn = [0]

        def fn():
            turn[0] = (turn[0] + 1) % len(sets)
            p, conf, ign, mc, gt = sets[turn[0]]
            ops.pl_stats(p, conf, ign, stats, N, BINS, 0.95, mc=mc if full else None, gt=gt if full else None)
        return fn
    keep = []
    for layout in ("random", "blocks", "single"):
        sets = [label_maps(layout, N, dev, gen) for _ in range(copies)]
        keep.append(sets)
        variants[f"{layout} all maps cold"], nbytes[f"{layout} all maps cold"] = launch(sets, True), 36 * n
        variants[f"{layout} no mc/gt cold"], nbytes[f"{layout} no mc/gt cold"] = launch(sets, False), 20 * n
        variants[f"{layout} all maps warm"], nbytes[f"{layout} all maps warm"] = launch(sets[:1], True), 36 * n
    ts = rounds_of(variants, rounds, launches)
    out = {k: summary(v, nbytes[k]) for k, v in ts.items()}
    for k, v in out.items():
        print(f"  N={N:3d} {k:24s} {v['us']:8.1f} us ({v['us_min']:.1f} .. {v['us_max']:.1f})  {v['bytes_per_s'] / 1e12:5.2f} TB/s",
              flush=True)
    out["copies_rotated_when_cold"] = copies
    out["single_over_random (all maps, cold)"] = round(out["single all maps cold"]["us"] / out["random all maps cold"]["us"], 2)
    out["blocks_over_random (all maps, cold)"] = round(out["blocks all maps cold"]["us"] / out["random all maps cold"]["us"], 2)
    return out


def time_step(steps, warmup, rounds, dev):
    from semivl_amd.model.builder import build_model
    from semivl_amd.monitor import PseudoLabelMeter
    from semivl_amd.synthetic import exp40_cfg, synthetic_batch
    from semivl_amd.train import FusedAdamW, semivl_train_step
    ops.set_gemm_emulation(6)
    cfg = exp40_cfg(B, S, 21, "pascal")
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev)
    opt = FusedAdamW(model, cfg["optimizer"])
    batch = synthetic_batch(B, S, 21, seed=1234, device=dev)
    batch["mask_u"] = torch.randint(0, 21, (B, S // 32, S // 32), device=dev).repeat_interleave(32, 1).repeat_interleave(32, 2)
    meter = PseudoLabelMeter(21, BINS, device=dev)
    it = 0
    for _ in range(warmup):
        semivl_train_step(model, batch, it, 1000, cfg, optimizer=opt)
        it += 1
    res = {"no meter": [], "meter": []}
    for _ in range(rounds):
        for name in res:
            mon = meter if name == "meter" else None
            semivl_train_step(model, batch, it, 1000, cfg, optimizer=opt, monitor=mon)     # the first step after the switch is not timed
            it += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                semivl_train_step(model, batch, it, 1000, cfg, optimizer=opt, monitor=mon)
                it += 1
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / steps * 1e3)
    rep = meter.report()
    out = {k: dict(ms_per_step=round(sorted(v)[len(v) // 2], 2), rounds=[round(x, 2) for x in v]) for k, v in res.items()}
    out["report"] = {k: round(float(rep[k]), 6) for k in ("mask_ratio", "guidance_coverage", "guidance_agreement", "pl_miou",
                                                           "train/loss")}
    out["report"]["steps"] = rep["steps"]
    for k, v in res.items():
        print(f"  {k:10s} {sorted(v)[len(v) // 2]:8.2f} ms/step  rounds {[round(x, 2) for x in v]}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "plstats_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, launches_per_round=a.launches,
               batch=f"{B} x {S}^2, {BINS} bins", kernel={})
    for name, N in (("VOC N=21", 21), ("ADE N=150", 150)):
        out["kernel"][name] = bench_kernel(N, a.rounds, a.launches, dev)
        torch.cuda.empty_cache()
    if not a.skip_step:
        out["step"] = dict(batch="16 + 16 x 512^2, VOC, mode 6, FusedAdamW", steps=a.steps, warmup=a.warmup,
                           rounds=a.step_rounds, **time_step(a.steps, a.warmup, a.step_rounds, dev))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
