"""MaskCLIP's refinements (ops.mc_refine: prompt denoising + key smoothing) pass by pass and as a whole, written to
profiles/maskclip_refine_times.json.

Shape: B = 4 images of 32 x 32 tokens (512^2 crops), keys E = 768, N = 21 (VOC) and N = 150 (ADE) classes, thresholds 0.5 / 0.7,
inputs from the recipe of the tests (cosines 0.2 + 0.03 N(0, 1), every third class 0.12 lower).

  passes   svl_mc_softmax_f32 (plain, and masked with the row maxima), svl_mc_class_peak_f32, svl_col_invsq_f32, the two
           svl_gemm_f32 products with the scaling between them (ops.mc_smooth) and svl_mc_select_f32, each alone, as warmed
           launches in alternating rounds between device events; `bytes` is what the pass must move (computed from the shape),
           `flop` what the products must compute.
  whole    ops.mc_refine: `warm` on the same inputs again and again (they stay in the 256 MiB Infinity Cache), `cold` rotating
           over copies of (x, k) that together exceed twice the cache, so every read of an input comes from HBM.
  mode     the GEMM arithmetic mode of the two products (0: exact fp32, 6: the split products where the library routes to them).

These times are context for the README, not gates.  usage: python tools/time_maskclip_refine.py [--rounds R] [--launches N]
[--out FILE.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402

CACHE_BYTES = 256 * 2 ** 20
B, HW, E = 4, 32 * 32, 768
PD, KS = 0.5, 0.7


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


def summary(ts, nbytes, flop=0):
    ms = ts[len(ts) // 2]
    out = dict(us=round(ms * 1e3, 2), us_min=round(ts[0] * 1e3, 2), us_max=round(ts[-1] * 1e3, 2), bytes=nbytes,
               gbytes_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1))
    if flop:
        out.update(flop=flop, tflop_per_s=round(flop / (ms * 1e-3) / 1e12, 2))
    return out


def inputs(N, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    low = torch.zeros(N, device=dev)
    low[2::3] = 0.12
    x = (0.2 + 0.03 * torch.randn(B * HW, N, device=dev, generator=g) - low).contiguous()
    return x, torch.randn(B * HW, E, device=dev, generator=g)


def bench(N, mode, rounds, launches, dev):
    ops.set_gemm_emulation(mode)
    x, k = inputs(N, dev, 0)
    rows, f = B * HW, 4
    P0, _ = ops.mc_softmax(x, B, HW, want_rowmax=False)
    peak = ops.mc_class_peak(P0, B, HW)
    P, rowmax = ops.mc_softmax(x, B, HW, peak, PD)
    s = ops.col_invsq(k, B, HW)
    O = ops.mc_smooth(P, k, s, B, HW)
    buf = ops.empty(rows, N, device=dev)
    out = ops.empty(B, N, HW, device=dev)
    passes = {
        "softmax_plain": (lambda: ops.mc_softmax(x, B, HW, want_rowmax=False, out=buf), 2 * rows * N * f, 0),
        "class_peak": (lambda: ops.mc_class_peak(P0, B, HW), (rows * N + B * N) * f, 0),
        "softmax_masked_rowmax": (lambda: ops.mc_softmax(x, B, HW, peak, PD, out=buf), (2 * rows * N + rows + B * N) * f, 0),
        "col_invsq": (lambda: ops.col_invsq(k, B, HW), (rows * E + B * E) * f, 0),
        "products": (lambda: ops.mc_smooth(P, k, s, B, HW), (2 * rows * E + 2 * rows * N + 4 * B * N * E + B * E) * f,
                     4 * rows * E * N),
        "select": (lambda: ops.mc_select(P, B, HW, O, rowmax, KS, out=out), (3 * rows * N + rows) * f, 0),
    }
    ts = rounds_of({n: p[0] for n, p in passes.items()}, rounds, launches)
    res = {n: summary(ts[n], passes[n][1], passes[n][2]) for n in passes}
    # the whole refinement: x and k in, the class planes out (intermediates stay on the chip's caches at this size)
    whole_bytes = (rows * N + rows * E + B * N * HW) * f
    copies = -(-2 * CACHE_BYTES // ((rows * N + rows * E) * f)) + 1
    ring = [inputs(N, dev, 1 + i) for i in range(copies)]
    state = dict(i=0)

    def cold():
        xi, ki = ring[state["i"] % copies]
        state["i"] += 1
        ops.mc_refine(xi, ki, B, HW, PD, KS, out=out)

    tw = rounds_of(dict(warm=lambda: ops.mc_refine(x, k, B, HW, PD, KS, out=out), cold=cold), rounds, launches)
    res["whole_warm"] = summary(tw["warm"], whole_bytes, 4 * rows * E * N)
    res["whole_cold"] = dict(summary(tw["cold"], whole_bytes, 4 * rows * E * N), copies=copies,
                             ring_bytes=copies * (rows * N + rows * E) * f)
    dropped = int((peak < PD).sum())
    res["case"] = dict(dropped_classes=dropped, smoothed_rows=round(float((rowmax < KS).float().mean()), 3),
                       hw2_flop_of_the_dense_form=2 * B * HW * HW * (E + N))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "maskclip_refine_times.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    res = dict(shape=dict(B=B, HW=HW, E=E, pd_thresh=PD, ks_thresh=KS), rounds=a.rounds, launches=a.launches,
               device=torch.cuda.get_device_name(0))
    try:
        for N in (21, 150):
            for mode in (0, 6):
                res[f"N{N}_mode{mode}"] = bench(N, mode, a.rounds, a.launches, dev)
                print(f"N {N} mode {mode}:", json.dumps({k: v.get("us") for k, v in res[f'N{N}_mode{mode}'].items() if "us" in v}))
    finally:
        ops.set_gemm_emulation(0)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
