"""Times the labelled cross-entropy launches at the VOC labelled branch (B = 16, N = 21, head resolution 128^2, crop 512^2):
the plain entry points and their label-smoothing / class-weight variants, on the same logits and label maps, alternating in
one process.  Each variant is warmed, then timed with device events over `--iters` launches, `--rounds` times in turn; the
JSON holds every round and the median.

    python tools/time_celoss.py --out profiles/celoss_kernel_times.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--nclass", type=int, default=21)
    ap.add_argument("--head", type=int, default=128)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_celoss: needs the GPU (a CPU run measures nothing)")
    from semivl_amd import ops
    dev = torch.device("cuda:0")
    B, N, h, S = a.batch, a.nclass, a.head, a.crop
    g = torch.Generator().manual_seed(1)
    low = (torch.randn(B, N, h, h, generator=g) * 2).to(dev)
    tgt = torch.randint(0, N, (B, S, S), generator=g)
    tgt[torch.rand(B, S, S, generator=g) < 0.1] = 255
    tgt = tgt.to(dev)
    cw = (torch.rand(N, generator=g) + 0.5).to(dev)
    full = ops.bilinear_planes_fwd(low, h, h, False, S, S)
    gs = torch.tensor([1.0 / (B * S * S), 0.0], device=dev)
    d_low, d_full = torch.empty_like(low), torch.empty_like(full)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    assert ops.ce_up_ok(B, N, h, h, S, S, False) and ops.ce_up_lsw_ok(B, N, h, h, S, S, False)
    settings = dict(plain={}, eps=dict(label_smoothing=0.1), weights=dict(class_weight=cw),
                    both=dict(label_smoothing=0.1, class_weight=cw))
    calls = {}
    for name, kw in settings.items():
        calls["ce_up_fused/" + name] = (lambda kw=kw: ops.ce_up_fused(low, S, S, False, tgt, True, dlogits=d_low, gscale=gs,
                                                                      sums_out=sums, **kw))
        calls["ce_fused/" + name] = (lambda kw=kw: ops.ce_fused(full, tgt, True, dlogits=d_full, gscale=gs, sums_out=sums, **kw))
    for f in calls.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.iters)
    res = dict(tool="time_celoss", device=torch.cuda.get_device_name(0), batch=B, nclass=N, head=h, crop=S, iters=a.iters,
               rounds=a.rounds, note="ms per call = the cross-entropy launch + svl_ce_finalize, device events; context, not a gate",
               ms_per_call={k: dict(median=round(statistics.median(v), 4), rounds=[round(x, 4) for x in v]) for k, v in times.items()})
    for fam in ("ce_up_fused", "ce_fused"):
        base = res["ms_per_call"][fam + "/plain"]["median"]
        res.setdefault("ratio_to_plain", {}).update({fam + "/" + s: round(res["ms_per_call"][fam + "/" + s]["median"] / base, 3)
                                                     for s in ("eps", "weights", "both")})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
