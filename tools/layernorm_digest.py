"""What the LayerNorm family of csrc/norm.hip and the two plane pack passes that share csrc/planes_split.h with it compute, bit
for bit, to compare two builds of the library: the seeded inputs and case lists of tests/rownorm_ref.py and
tests/test_vit_onepass_gpu.py (the smallest shapes that reach each path, hostile rows included), every entry point called
through the C ABI on NaN- or sentinel-prefilled outputs (an element a kernel leaves unwritten shows), and one SHA-256 per (entry
point, shape) over every output of every call on it written to a JSON file.  One build per process; command line, `sha` and
`compare` are tools/pixel_loss_digest.py's.
usage: python tools/layernorm_digest.py [--root TREE] --out FILE.json
       python tools/layernorm_digest.py --compare A.json B.json"""
import hashlib
import os
import sys

import torch

from pixel_loss_digest import main, sha

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))


def run(d):
    import rownorm_ref as R
    import test_vit_onepass_gpu as T
    from semivl_amd import ops, lib as L
    lib, p, st = L.load(), ops._p, ops._st
    out = {}

    def nans(*shape):
        return torch.full(shape, float("nan"), device=d)

    def put(key, variant="", **tensors):
        """One digest per (entry point, shape): the SHA-256 over (variant, name, SHA-256) of every output of every call on it."""
        h = out.setdefault(key, hashlib.sha256())
        for n, t in tensors.items():
            if t is not None:
                h.update(f"{variant}/{n}={sha(t)};".encode())

    def packed(key, variant, pb):
        put(key, variant, planes=pb.buf, sexp=pb.sexp, rnorm=pb.rnorm, amax=pb.amax)

    # ---- the row kernels on the shapes of tests/test_rownorm_kernels_gpu.py
    for rows, C in [(r, c) for c in R.LN_FWD_C for r in R.LN_FWD_ROWS] + [R.LN_FWD_BIG]:
        x, _, _, gamma, beta, eps = (t.to(d) if torch.is_tensor(t) else t for t in R.ln_inputs(rows, C))
        y, stats = nans(rows, C), nans(rows, 2)
        L.check(lib.svl_layernorm_fwd(p(x), p(gamma), p(beta), eps, rows, C, p(y), p(stats), st()), "fwd")
        put(f"fwd/r{rows}_C{C}", y=y, stats=stats)
    for rows, C in [(r, c) for c in R.LN_PLANES_C for r in R.LN_PLANES_ROWS] + [R.LN_PLANES_BIG]:
        x, _, _, gamma, beta, eps = (t.to(d) if torch.is_tensor(t) else t for t in R.ln_inputs(rows, C))
        prow = ops.planes_rows(rows)
        for fmt, per_row in (("bf16x3", 48), ("f16x2", 32)):
            for want_y in (True, False):
                y, stats = (nans(rows, C) if want_y else None), nans(rows, 2)
                planes = torch.full((C // 16 * prow * per_row,), 0x4240, dtype=torch.int16, device=d)
                sexp = torch.full((prow,), 77, dtype=torch.int32, device=d)
                rnorm = torch.full((prow,), T.SENT, device=d)
                if fmt == "bf16x3":
                    L.check(lib.svl_layernorm_fwd_planes(p(x), p(gamma), p(beta), eps, rows, C, p(y), p(stats), p(planes), prow, st()), fmt)
                else:
                    L.check(lib.svl_layernorm_fwd_planes_f16x2(p(x), p(gamma), p(beta), eps, rows, C, p(y), p(stats), p(planes), prow,
                                                               p(sexp), p(rnorm), st()), fmt)
                put(f"fwd_planes_{fmt}/r{rows}_C{C}", f"y{int(want_y)}", y=y, stats=stats, planes=planes, sexp=sexp, rnorm=rnorm)
    for rows, C in [(r, c) for c in R.LN_BWD_C for r in R.LN_BWD_ROWS + R.LN_BWD_ROWS_PARTS] + [R.LN_BWD_BIG]:
        x, dy, add, gamma, beta, eps = (t.to(d) if torch.is_tensor(t) else t for t in R.ln_inputs(rows, C))
        stats = nans(rows, 2)
        L.check(lib.svl_layernorm_fwd(p(x), p(gamma), p(beta), eps, rows, C, p(nans(rows, C)), p(stats), st()), "fwd")
        nparts = lib.svl_layernorm_bwd_parts(rows)
        for with_add in (True, False):
            for parts in (True, False):
                dx, dg, db = nans(rows, C), (nans(nparts, C) if parts else None), (nans(nparts, C) if parts else None)
                L.check(lib.svl_layernorm_bwd(p(dy), p(x), p(stats), p(gamma), rows, C, p(add if with_add else None), p(dx), p(dg), p(db),
                                              st()), "bwd")
                put(f"bwd/r{rows}_C{C}", f"add{int(with_add)}_parts{int(parts)}", dx=dx, dgamma_part=dg, dbeta_part=db)

    # ---- the C = 768 pack kernels on the cases of tests/test_vit_onepass_gpu.py
    for rows, variant, row_off, want_y in T.FWD_PARAMS:
        x, _, _, gamma, beta = (t.to(d) for t in T._inputs(rows, T.K768, variant))
        for row_rnorm in (0, 1):
            for ro in sorted({row_off, 0, 32}):
                for with_amax in (True, False):
                    pb = T._PackBufs(rows, T.K768, ro, d)
                    y, stats = (nans(rows, T.K768) if want_y else None), nans(rows, 2)
                    L.check(lib.svl_layernorm_fwd_pack_f16x2(p(x), p(gamma), p(beta), T.EPS, rows, T.K768, p(y), p(stats), p(pb.buf), pb.prow,
                                                             ro, p(pb.sexp), p(pb.rnorm), row_rnorm, p(pb.amax) if with_amax else None,
                                                             st()), "fwd_pack")
                    key, var = f"fwd_pack/r{rows}_{variant}_off{row_off}_y{int(want_y)}", f"off{ro}_rowrnorm{row_rnorm}_amax{int(with_amax)}"
                    put(key, var, y=y, stats=stats)
                    packed(key, var, pb)
    for rows, variant, row_off in T.FWD_CASES:
        x, dy, add, gamma, beta = (t.to(d) for t in T._inputs(rows, T.K768, variant))
        stats = nans(rows, 2)
        L.check(lib.svl_layernorm_fwd(p(x), p(gamma), p(beta), T.EPS, rows, T.K768, p(nans(rows, T.K768)), p(stats), st()), "fwd")
        for with_add in (True, False):
            pb, dx = T._PackBufs(rows, T.K768, row_off, d), nans(rows, T.K768)
            L.check(lib.svl_layernorm_bwd_pack_f16x2(p(dy), p(x), p(stats), p(gamma), rows, T.K768, p(add if with_add else None), p(dx),
                                                     p(pb.buf), pb.prow, row_off, p(pb.sexp), p(pb.rnorm), p(pb.amax), st()), "bwd_pack")
            key = f"bwd_pack/r{rows}_{variant}_off{row_off}"
            put(key, f"add{int(with_add)}", dx=dx)
            packed(key, f"add{int(with_add)}", pb)

    # ---- the generic pack passes: (rows, K, ld, k_stride); k_stride > 1 reads a [K, rows] matrix as its transpose
    shapes = [s + (1,) for s in next(m for m in T.test_split_planes_tensor_amax.pytestmark if m.name == "parametrize").args[1]]
    shapes += [(40, 64, 67, 1), (70, 48, 1, 70), (768, 768, 768, 1)]
    g = torch.Generator().manual_seed(31)
    for rows, K, ld, ks in shapes:
        src = (torch.randn(K, rows, generator=g) if ks > 1 else torch.randn(rows, ld, generator=g)).to(d)
        for ro in (0, 32):
            pb = T._PackBufs(rows, K, ro, d)
            L.check(lib.svl_split_planes_f16x2(p(src), ld, ks, rows, K, p(pb.buf), pb.prow, ro, p(pb.sexp), p(pb.rnorm), p(pb.amax), st()),
                    "split h2")
            packed(f"split_f16x2/r{rows}_K{K}_ld{ld}_ks{ks}", f"off{ro}", pb)
            planes = torch.full((K // 16 * pb.prow * 48,), 0x4240, dtype=torch.int16, device=d)
            L.check(lib.svl_split_planes_bf16x3(p(src), ld, ks, rows, K, p(planes), pb.prow, ro, st()), "split bf16x3")
            put(f"split_bf16x3/r{rows}_K{K}_ld{ld}_ks{ks}", f"off{ro}", planes=planes)
    torch.cuda.synchronize()
    return {k: h.hexdigest() for k, h in out.items()}


if __name__ == "__main__":
    sys.exit(main(run, "layernorm_digest"))
