"""Standalone times of the LayerNorm -> planes kernels at [32800, 768] against the sequences they replace (device events,
warm, 4 rotating buffer sets of ~0.4 GB each so that inputs do not sit in L2 / MALL from the previous call)."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from semivl_amd import ops, lib as L
lib = L.load()
dev = torch.device("cuda:0")
rows, Cc, EPS, NSET = 32800, 768, 1e-5, 4
p, st = ops._p, ops._st
torch.manual_seed(0)
gamma = (1 + 0.3 * torch.randn(Cc)).to(dev); beta = (0.2 * torch.randn(Cc)).to(dev)
prow = ops.planes_rows(rows)
sets = []
for i in range(NSET):
    s = dict(x=torch.randn(rows, Cc, device=dev) * 3 + 0.5, dy=torch.randn(rows, Cc, device=dev), add=torch.randn(rows, Cc, device=dev),
             y=torch.empty(rows, Cc, device=dev), stats=torch.empty(rows, 2, device=dev),
             buf=torch.empty(Cc // 16 * prow * 32, dtype=torch.float16, device=dev), sexp=torch.empty(prow, dtype=torch.int32, device=dev),
             rnorm=torch.empty(prow, device=dev), amax=torch.zeros(1, dtype=torch.int32, device=dev))
    L.check(lib.svl_layernorm_fwd(p(s["x"]), p(gamma), p(beta), EPS, rows, Cc, p(s["y"]), p(s["stats"]), st()))
    sets.append(s)

def split(s, src):
    L.check(lib.svl_split_planes_f16x2(p(src), Cc, 1, rows, Cc, p(s["buf"]), prow, 0, p(s["sexp"]), p(s["rnorm"]), None, st()))

def fwd_y_old(s):
    L.check(lib.svl_layernorm_fwd(p(s["x"]), p(gamma), p(beta), EPS, rows, Cc, p(s["y"]), p(s["stats"]), st())); split(s, s["y"])
def fwd_y_new(s):
    L.check(lib.svl_layernorm_fwd_pack_f16x2(p(s["x"]), p(gamma), p(beta), EPS, rows, Cc, p(s["y"]), p(s["stats"]), p(s["buf"]), prow, 0,
                                             p(s["sexp"]), p(s["rnorm"]), 0, p(s["amax"]), st()))
def fwd_p_old(s):
    L.check(lib.svl_layernorm_fwd_planes_f16x2(p(s["x"]), p(gamma), p(beta), EPS, rows, Cc, None, p(s["stats"]), p(s["buf"]), prow,
                                               p(s["sexp"]), p(s["rnorm"]), st()))
def fwd_p_new(s):
    L.check(lib.svl_layernorm_fwd_pack_f16x2(p(s["x"]), p(gamma), p(beta), EPS, rows, Cc, None, p(s["stats"]), p(s["buf"]), prow, 0,
                                             p(s["sexp"]), p(s["rnorm"]), 1, None, st()))
def fwd_row_only(s):
    L.check(lib.svl_layernorm_fwd(p(s["x"]), p(gamma), p(beta), EPS, rows, Cc, p(s["y"]), p(s["stats"]), st()))
def pack_only(s):
    split(s, s["y"])
def mk_bwd(new, add):
    def f(s):
        a = p(s["add"]) if add else None
        if new:
            L.check(lib.svl_layernorm_bwd_pack_f16x2(p(s["dy"]), p(s["x"]), p(s["stats"]), p(gamma), rows, Cc, a, p(s["y"]), p(s["buf"]),
                                                     prow, 0, p(s["sexp"]), p(s["rnorm"]), None, st()))
        else:
            L.check(lib.svl_layernorm_bwd(p(s["dy"]), p(s["x"]), p(s["stats"]), p(gamma), rows, Cc, a, p(s["y"]), None, None, st()))
            split(s, s["y"])
    return f

def time_us(f, n=100):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        f(sets[i % NSET])
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n

cases = [("row kernel alone (svl_layernorm_fwd)", fwd_row_only, None), ("pack pass alone (svl_split_planes_f16x2)", pack_only, None),
         ("fwd, y + planes", fwd_y_old, fwd_y_new), ("fwd, planes only", fwd_p_old, fwd_p_new),
         ("bwd + dx_add, dx + planes", mk_bwd(False, True), mk_bwd(True, True)), ("bwd, dx + planes", mk_bwd(False, False), mk_bwd(True, False))]
print(torch.cuda.get_device_name(0), flush=True)
for name, old, new in cases:
    fs = [f for f in (old, new) if f]
    for f in fs:
        time_us(f, 20)
    res = [[] for _ in fs]
    for rep in range(7):
        for k, f in enumerate(fs):
            res[k].append(time_us(f))
    line = f"{name:45s} old: median {statistics.median(res[0]):7.1f} us (min {min(res[0]):.1f}, max {max(res[0]):.1f})"
    if new:
        line += f"   new: median {statistics.median(res[1]):7.1f} us (min {min(res[1]):.1f}, max {max(res[1]):.1f})"
    print(line, flush=True)
