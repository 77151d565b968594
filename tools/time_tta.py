"""Test-time augmentation: what one view costs the evaluator's running mean.  One VOC-sized target (1 x 21 x 366 x 500) and
one ADE-sized target (1 x 150 x 512 x 683), the six mmseg ratios (0.5 .. 1.75) unflipped and flipped: for every view, the
view's logits at its own size are folded into the target by

  fused     ops.tta_accum (svl_tta_accum_f32): one launch, the destination read once and written once
  composed  what it replaces: ops.bilinear_planes_fwd -> ops.softmax_planes -> a flip (ATen) -> ops.add: four passes over
            [B, N, H, W] tensors (the flip only for the mirrored views)

as warmed launches in alternating rounds between device events.  Written to profiles/tta_times.json with the fused kernel's
rate on its own bytes: 4 N H W written, the same again read (accumulate = 1, as in every view but the first), plus the source
read once.  The VOC destination (15 MB) fits the 256 MiB Infinity Cache and the 32 MiB of L2 with room to spare and the ADE
destination (210 MB) largely fits the Infinity Cache, and the same buffers are used launch after launch: these are rates of
cache-resident traffic, NOT HBM rates, and are labelled so.

usage: python tools/time_tta.py [--rounds R] [--launches N] [--out FILE.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402

RATIOS = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
CASES = (("VOC 1x21x366x500", 21, 366, 500), ("ADE 1x150x512x683", 150, 512, 683))
CACHE_BYTES = 256 * 2 ** 20


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


def stat(ts):
    return dict(us=round(ts[len(ts) // 2] * 1e3, 2), us_min=round(ts[0] * 1e3, 2), us_max=round(ts[-1] * 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "tta_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    out = dict(tool="tools/time_tta.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, launches_per_round=a.launches,
               kind="0 (logits), align_corners=False, scale=1/12, accumulate=1", cases={})
    for name, N, H, W in CASES:
        acc = torch.rand(1, N, H, W, device=dev, generator=gen)
        tmp_up, tmp_p = torch.empty_like(acc), torch.empty_like(acc)
        dst_bytes = 4 * N * H * W
        res = dict(destination_bytes=dst_bytes,
                   residency="destination fits the Infinity Cache (and is reused launch after launch): cache-resident rate"
                   if 3 * dst_bytes < CACHE_BYTES else
                   "destination (x3 with the composition's temporaries) exceeds the Infinity Cache only in the composed form; "
                   "the fused form's single destination largely fits it: a largely cache-resident rate, not an HBM rate",
                   views={})
        tot_f = tot_c = 0.0
        for r in RATIOS:
            h, w = int(H * r + 0.5), int(W * r + 0.5)
            src = torch.randn(1, N, h, w, device=dev, generator=gen) * 4
            for flip in (False, True):
                def fused():
                    ops.tta_accum(src, acc, 0, False, flip, 1.0 / 12.0, True)

                def composed():
                    ops.bilinear_planes_fwd(src, h, w, False, H, W, out=tmp_up)
                    p = ops.softmax_planes(tmp_up, out=tmp_p)
                    ops.add(acc, p.flip(3) if flip else p, out=acc)
                ts = rounds_of({"fused": fused, "composed": composed}, a.rounds, a.launches)
                acc.fill_(0.5)                                  # (keeps the running sum finite over thousands of launches)
                f, c = stat(ts["fused"]), stat(ts["composed"])
                nbytes = 2 * dst_bytes + 4 * N * h * w
                f["own_bytes"] = nbytes
                f["own_bytes_per_s_cache_resident"] = round(nbytes / (f["us"] * 1e-6))
                res["views"][f"ratio {r} flip {int(flip)} ({h}x{w})"] = dict(fused=f, composed=c)
                tot_f, tot_c = tot_f + f["us"], tot_c + c["us"]
                print(f"  {name} r={r} flip={int(flip)}: fused {f['us']:8.1f} us ({nbytes / (f['us'] * 1e-6) / 1e12:5.2f} TB/s own bytes, "
                      f"cache-resident), composed {c['us']:8.1f} us", flush=True)
        res["twelve_views_us"] = dict(fused=round(tot_f, 1), composed=round(tot_c, 1))
        out["cases"][name] = res
        del acc, tmp_up, tmp_p
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
