"""The evaluation report's kernel beside the evaluator's histogram, written to profiles/confusion_times.json:

  kernel     svl_confusion_i64 beside svl_iou_hist_i64 (what `evaluate` launches) on the same 16 x 512^2 int64 maps (16 B per
             pixel), as warmed launches in alternating rounds between device events.  Maps: `random` (every pixel its own
             class: many pair keys per wave, no contention), `blocks` (piecewise constant, 32 x 32 cells: what a segmentation
             map looks like) and `single` (one class everywhere: every lane of every wave on one counter).  Every K is timed in
             BOTH forms where the table fits the 160 KB of LDS -- `lds` (block-private 32-bit counters) and `global` (the waves'
             counts straight into 64-bit atomics), forced through svl_set_confusion_lds_max_classes -- which is what places
             svl_confusion_lds_max_classes().  `cold`: the launches rotate over copies of the maps that together exceed the
             256 MiB Infinity Cache twice, so every read comes from HBM; `warm`: the same 67 MB again and again.
  evaluator  ms per image of report.evaluate_report (no files) and evaluate.evaluate on one loader of 512^2 images through
             the VOC model (random weights, mode 'original'), alternating.

usage: python tools/time_confusion.py [--rounds R] [--launches N] [--images I] [--out FILE.json] [--skip-eval]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import lib as L  # noqa: E402
from semivl_amd import ops  # noqa: E402

PEAK = 8.0e12
CACHE_BYTES = 256 * 2 ** 20
B, S = 16, 512
LDS_HW_MAX = 201


def rounds_of(variants, rounds, launches):
    """{name: sorted ms per launch over the rounds}; the variants alternate inside every round."""
    for fn in variants.values():
        for _ in range(3):
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


def label_maps(layout, K, dev, gen):
    """(pred, target) of one batch: the prediction agrees with the annotation on ~70 % of the pixels; 40 rows are ignored."""
    if layout == "random":
        t = torch.randint(0, K, (B, S, S), device=dev, generator=gen)
        p = torch.where(torch.rand(B, S, S, device=dev, generator=gen) < 0.7, t,
                        torch.randint(0, K, (B, S, S), device=dev, generator=gen))
    elif layout == "blocks":
        cells = lambda: torch.randint(0, K, (B, S // 32, S // 32), device=dev, generator=gen).repeat_interleave(32, 1).repeat_interleave(32, 2)
        t = cells()
        p = torch.where(torch.rand(B, S // 32, S // 32, device=dev, generator=gen).repeat_interleave(32, 1).repeat_interleave(32, 2) < 0.7,
                        t, cells())
    else:
        t = torch.full((B, S, S), K // 2, dtype=torch.int64, device=dev)
        p = t.clone()
    if layout != "single":
        t[:, -40:, :] = 255
    return p.contiguous(), t.contiguous()


def bench_kernel(K, rounds, launches, dev, warm):
    lib = L.load()
    gen = torch.Generator(device=dev).manual_seed(K)
    n = B * S * S
    copies = -(-2 * CACHE_BYTES // (16 * n)) + 1
    table = ops.zeros(ops.confusion_len(K), dtype=torch.int64, device=dev)
    hist = ops.zeros(3 * K, dtype=torch.int64, device=dev)
    forms = (("lds", LDS_HW_MAX), ("global", 0)) if K <= LDS_HW_MAX else (("global", 0),)
    variants = {}

    def conf_fn(sets, bound):
        turn = [0]

        def fn():
            turn[0] = (turn[0] + 1) % len(sets)
            lib.svl_set_confusion_lds_max_classes(bound)
            ops.confusion(sets[turn[0]][0], sets[turn[0]][1], K, 255, table)
        return fn

    def hist_fn(sets):
        turn = [0]

        def fn():
            turn[0] = (turn[0] + 1) % len(sets)
            ops.iou_hist(sets[turn[0]][0], sets[turn[0]][1], K, 255, hist)
        return fn
    keep = []
    for layout in ("random", "blocks", "single"):
        sets = [label_maps(layout, K, dev, gen) for _ in range(copies)]
        keep.append(sets)
        for form, bound in forms:
            variants[f"{layout} confusion {form} cold"] = conf_fn(sets, bound)
            if warm:
                variants[f"{layout} confusion {form} warm"] = conf_fn(sets[:1], bound)
        variants[f"{layout} iou_hist cold"] = hist_fn(sets)
        if warm:
            variants[f"{layout} iou_hist warm"] = hist_fn(sets[:1])
    try:
        ts = rounds_of(variants, rounds, launches)
    finally:
        lib.svl_set_confusion_lds_max_classes(-1)
    out = {k: summary(v, 16 * n) for k, v in ts.items()}
    for k, v in out.items():
        print(f"  K={K:4d} {k:32s} {v['us']:9.1f} us ({v['us_min']:.1f} .. {v['us_max']:.1f})  {v['bytes_per_s'] / 1e12:5.2f} TB/s",
              flush=True)
    out["copies_rotated_when_cold"] = copies
    out["lds_table_bytes"] = 4 * (K + 1) ** 2
    for form, _ in forms:
        r = out[f"random confusion {form} cold"]["us"]
        out[f"single_over_random ({form}, cold)"] = round(out[f"single confusion {form} cold"]["us"] / r, 2)
        out[f"blocks_over_random ({form}, cold)"] = round(out[f"blocks confusion {form} cold"]["us"] / r, 2)
    return out


def time_evaluator(images, rounds, dev):
    from semivl_amd.evaluate import evaluate
    from semivl_amd.model.builder import build_model
    from semivl_amd.report import evaluate_report
    from semivl_amd.synthetic import exp40_cfg
    ops.set_gemm_emulation(6)
    cfg = dict(exp40_cfg(1, S, 21, "pascal"), clip_encoder=None)
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev)
    g = torch.Generator().manual_seed(7)
    loader = [(torch.randn(1, 3, S, S, generator=g),
               torch.randint(0, 21, (1, S // 32, S // 32), generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2), None)
              for _ in range(images)]
    runs = {"evaluate": lambda: evaluate(model, loader, "original", cfg),
            "evaluate_report": lambda: evaluate_report(model, loader, "original", cfg)}
    for fn in runs.values():
        fn()
    res = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / images * 1e3)
    m, _ = runs["evaluate"]()
    rep = runs["evaluate_report"]()
    assert rep.miou == m, (rep.miou, m)
    out = {k: dict(ms_per_image=round(sorted(v)[len(v) // 2], 3), rounds=[round(x, 3) for x in v]) for k, v in res.items()}
    for k, v in out.items():
        print(f"  {k:16s} {v['ms_per_image']:8.3f} ms/image  rounds {v['rounds']}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--eval-rounds", type=int, default=3)
    ap.add_argument("--classes", type=int, nargs="+", default=[21, 127, 128, 150, 201, 202])
    ap.add_argument("--skip-eval", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "confusion_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, launches_per_round=a.launches,
               batch=f"{B} x {S}^2 int64 maps, 16 B per pixel", lds_max_classes=int(L.load().svl_confusion_lds_max_classes()),
               kernel={})
    for K in a.classes:
        out["kernel"][f"K={K}"] = bench_kernel(K, a.rounds, a.launches, dev, warm=K in (21, 150))
        torch.cuda.empty_cache()
    if not a.skip_eval:
        out["evaluator"] = dict(images=a.images, size=f"1 x 3 x {S}^2, VOC model, mode 'original', bf16x6 GEMMs",
                                rounds=a.eval_rounds, **time_evaluator(a.images, a.eval_rounds, dev))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
