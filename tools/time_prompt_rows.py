"""us per launch of the prompt-row kernels at VOC B = 32 (32 x 1025 x 768 floats, P = 10): the expand form of svl_prompt_rows_fwd_f32
against svl_copy2d_f32 on the same bytes, the in-place form and the two backward forms, three alternating rounds of 20 launches
each.  Prints one JSON line (profiles/prompt_rows_rate.json).
usage: python tools/time_prompt_rows.py"""
import json
import os
import sys

import torch


sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from semivl_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
B, T, P, E = 32, 1025, 10, 768
src = torch.randn(B * T, E, device=dev)
emb = torch.randn(P, E, device=dev)
mask = (torch.rand(B, P, E, device=dev) < 0.9).float()
dst = torch.empty(B * (T + P), E, device=dev)
cp = torch.empty(B * T, E, device=dev)
dxo = torch.empty(B * T, E, device=dev)
demb = torch.empty(P, E, device=dev)


def t(fn, n=20):
    for _ in range(3):
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
    expand=lambda: ops.prompt_rows_fwd(emb, B, P, dst, src=src, mask=mask, scale=1 / 0.9),
    copy2d=lambda: ops.copy2d(src, 0, B * T, 0, E, cp, 0, B * T, 0, E, B * T, E),
    inplace=lambda: ops.prompt_rows_fwd(emb, B, P, dst, mask=mask, scale=1 / 0.9),
    bwd_zero=lambda: ops.prompt_rows_bwd(dst, B, P, out=demb, mask=mask, scale=1 / 0.9),
    bwd_compact=lambda: ops.prompt_rows_bwd(dst, B, P, out=demb, mask=mask, scale=1 / 0.9, compact=dxo))
res = {k: [] for k in fns}
for rep in range(3):
    for k, fn in fns.items():
        res[k].append(round(t(fn), 2))
out = dict(shape=[B, T, P, E], us=res, bytes_expand=4 * E * B * (2 * T + P), bytes_copy2d=8 * E * B * T)
out["GBps_expand"] = round(out["bytes_expand"] / min(res["expand"]) / 1e3, 1)
out["GBps_copy2d"] = round(out["bytes_copy2d"] / min(res["copy2d"]) / 1e3, 1)
print(json.dumps(out))
