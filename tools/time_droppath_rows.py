"""us per launch of the two stochastic-depth kernels at VOC B = 32 (32 x 1025 rows x 768 floats, keep 0.9, every fourth sample
dropped and none dropped): svl_droppath_fwd_f32 into a third buffer and in place in the branch's buffer, svl_droppath_bwd_f32,
and svl_copy2d_f32 on the same matrix (one read, one write) as the yardstick; three alternating rounds of 50 warmed launches
each between device events.  Bytes per launch are what the kernel has to move: 12 per element forward and 8 backward with no
sample dropped; a dropped sample's rows cost one read less.  Prints one JSON line (profiles/droppath_rows_rate.json).
usage: python tools/time_droppath_rows.py"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
B, T, E, KEEP = 32, 1025, 768, 0.9
branch = torch.randn(B * T, E, device=dev)
work = branch.clone()
resid = torch.randn(B * T, E, device=dev)
out = torch.empty(B * T, E, device=dev)
cp = torch.empty(B * T, E, device=dev)
ones = torch.ones(B, device=dev)
some = torch.tensor([0.0 if b % 4 == 3 else 1.0 for b in range(B)], device=dev)
ndrop = int((some == 0).sum())


def t(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


fns = dict(
    fwd_keep_all=lambda: ops.droppath_add(branch, resid, ones, KEEP, B, T, out=out),
    fwd_inplace_keep_all=lambda: ops.droppath_add(work, resid, ones, KEEP, B, T),
    fwd_drop_quarter=lambda: ops.droppath_add(branch, resid, some, KEEP, B, T, out=out),
    bwd_keep_all=lambda: ops.droppath_scale(branch, ones, KEEP, B, T),
    bwd_drop_quarter=lambda: ops.droppath_scale(branch, some, KEEP, B, T),
    copy2d=lambda: ops.copy2d(branch, 0, B * T, 0, E, cp, 0, B * T, 0, E, B * T, E))
n = B * T * E
nbytes = dict(fwd_keep_all=12 * n, fwd_inplace_keep_all=12 * n, fwd_drop_quarter=12 * n - 4 * ndrop * T * E, bwd_keep_all=8 * n,
              bwd_drop_quarter=8 * n - 4 * ndrop * T * E, copy2d=8 * n)
res = {k: [] for k in fns}
for rep in range(3):
    for k, fn in fns.items():
        res[k].append(round(t(fn), 2))
out_ = dict(tool="time_droppath_rows", device=torch.cuda.get_device_name(0), shape=[B, T, E], keep=KEEP, dropped_samples=ndrop,
            launches_per_round=50, us=res, bytes=nbytes, GBps={k: round(nbytes[k] / min(v) / 1e3, 1) for k, v in res.items()})
print(json.dumps(out_))
