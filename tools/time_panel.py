"""The debug panel's two kernels and the whole capture, written to profiles/panel_times.json:

  kernels  svl_panel_image_u8 and svl_panel_label_u8 on one tile of the VOC step (B = 16, 512 x 512) inside the guided canvas
           [16, 2048, 2048, 3], as warmed launches in alternating rounds between device events.  `warm`: the same input
           again and again (50 MB of fp32 / 34 MB of int64: it stays in the 256 MiB Infinity Cache); `cold`: the launches
           rotate over copies of the input that together exceed that cache twice, so every read comes from HBM.  Bytes
           moved = input read once + tile written once (the canvas bytes are written, never read).
  capture  StepPanel.render of the guided figure (4 image tiles + 12 label tiles per sample: 16 launches) between device
           events, and separately on the host: the asynchronous copy of the canvas to pinned memory (201 MB, device
           events around it) and the PNG encoding of the 16 files in the writer threads (wall time of close()).

usage: python tools/time_panel.py [--rounds R] [--launches N] [--out FILE.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402
from semivl_amd.data import MEAN, STD  # noqa: E402
from semivl_amd.panel import StepPanel, canvas_shape  # noqa: E402

PEAK = 8.0e12
CACHE_BYTES = 256 * 2 ** 20
B, S, K = 16, 512, 21


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


def summary(ts, nbytes, **more):
    ms = ts[len(ts) // 2]
    rate = nbytes / (ms * 1e-3)
    return dict(us=round(ms * 1e3, 2), us_min=round(ts[0] * 1e3, 2), us_max=round(ts[-1] * 1e3, 2), bytes=nbytes,
                bytes_per_s=round(rate), fraction_of_8TBps_peak=round(rate / PEAK, 3), **more)


def rotating(copies):
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % len(copies)
        return copies[state["i"]]
    return nxt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "panel_times.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    canvas = torch.empty(canvas_shape(B, S, S, True), dtype=torch.uint8, device=dev)
    img = torch.randn(B, 3, S, S, generator=g).to(dev)
    small = torch.randint(0, K, (B, S // 32, S // 32), generator=g)
    lab = small.repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous().to(dev)
    pal = torch.randint(0, 256, (K, 3), generator=g).to(torch.uint8).to(dev)
    tile = B * S * S * 3
    n_img = 2 * CACHE_BYTES // (img.numel() * 4) + 1
    n_lab = 2 * CACHE_BYTES // (lab.numel() * 8) + 1
    imgs, labs = [img.clone() for _ in range(n_img)], [lab.clone() for _ in range(n_lab)]
    next_img, next_lab = rotating(imgs), rotating(labs)
    variants = {
        "image_warm": lambda: ops.panel_image(img, MEAN, STD, canvas, 0, S),
        "image_cold": lambda: ops.panel_image(next_img(), MEAN, STD, canvas, 0, S),
        "label_warm": lambda: ops.panel_label(lab, pal, canvas, S, S),
        "label_cold": lambda: ops.panel_label(next_lab(), pal, canvas, S, S),
    }
    ts = rounds_of(variants, args.rounds, args.launches)
    out = dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, S=S, K=K, canvas=list(canvas.shape)),
               rounds=args.rounds, launches=args.launches, kernels={})
    for name, t in ts.items():
        nbytes = (img.numel() * 4 if name.startswith("image") else lab.numel() * 8) + tile
        out["kernels"][name] = summary(t, nbytes, inputs_cache_resident=name.endswith("warm"),
                                       copies=1 if name.endswith("warm") else (n_img if name.startswith("image") else n_lab))
    del imgs, labs
    # the whole capture: 16 tiles per sample
    images = [torch.randn(B, 3, S, S, generator=g).to(dev) for _ in range(4)]
    maps = [lab.roll(i, 1).contiguous() for i in range(11)]
    rows = [maps[0:4], maps[4:8], [None] + maps[8:11]]
    with tempfile.TemporaryDirectory() as tmp:
        panel = StepPanel(tmp, workers=2)
        t = rounds_of({"render": lambda: panel.render(images, rows)}, args.rounds, 3)["render"]
        read = sum(i.numel() * 4 for i in images) + 12 * lab.numel() * 8
        out["capture"] = dict(render=summary(t, read + canvas.numel(), launches=16, inputs_cache_resident=False,
                                             note="16 distinct inputs of 50 / 34 MB each: 604 MB read per render, beyond the cache"))
        cv = panel.render(images, rows)
        host = torch.empty(cv.shape, dtype=torch.uint8, pin_memory=True)
        copies = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            host.copy_(cv, non_blocking=True)
            e1.record()
            e1.synchronize()
            copies.append(e0.elapsed_time(e1))
        copies.sort()
        out["capture"]["copy_to_pinned_host"] = dict(ms=round(copies[len(copies) // 2], 3), bytes=cv.numel(),
                                                     bytes_per_s=round(cv.numel() / (copies[len(copies) // 2] * 1e-3)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        panel.capture(0, images, rows)
        t_step = time.perf_counter() - t0
        panel.close()
        t_all = time.perf_counter() - t0
        out["capture"]["host"] = dict(step_thread_ms=round(t_step * 1e3, 2), until_files_written_ms=round(t_all * 1e3, 1),
                                      files=B, png_bytes=sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp)),
                                      workers=2, note="step_thread_ms: what the training thread spends in capture() (16 launches, "
                                      "pinned allocation, copy enqueue); the rest is PNG encoding in the writer threads")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
