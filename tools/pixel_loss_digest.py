"""What the pixel-loss family and the kernels that share its bilinear index (csrc/bilinear_index.h) compute, bit for bit, to
compare two builds of the library: seeded CPU-generated inputs at the smallest shapes that reach every code path, every
kernel called through semivl_amd.ops, and the SHA-256 of every output tensor written to a JSON file.  One build per process
(--root picks the tree whose semivl_amd is imported); --compare fails on any digest that differs or is missing.
usage: python tools/pixel_loss_digest.py [--root TREE] --out FILE.json
       python tools/pixel_loss_digest.py --compare A.json B.json"""
import argparse
import hashlib
import json
import os
import sys

import torch

# (N, HW) of the full-resolution kernels: vector path with P = 256; HW % 4 != 0 (scalar path); P = 128 (two threads per
# pixel); P = 64 (four threads per pixel) with a ragged last block
FULL = [(21, 672), (5, 63), (81, 320), (150, 200)]
# (N, h, w, H, W) of the resize-fused kernels: one tile at ratio 4; ragged tiles at a non-integer ratio; ratio 1; ratio 2,
# ragged; many classes; the widest staged tile
UP = [(5, 8, 8, 32, 32), (7, 13, 20, 50, 79), (3, 9, 9, 9, 9), (4, 17, 11, 34, 22), (81, 16, 16, 64, 64), (150, 24, 40, 96, 160)]
# the kernels that only include the index header
INDEX_ONLY = [(7, 13, 20, 50, 79), (3, 9, 9, 9, 9)]
B = 2


def sha(t):
    t = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def maps(g, N, shape):
    """Label maps of `shape` = (B, ...) on the CPU: targets with 255s, confidences, an `ign` band, a guidance map that is
    half 255, per-image weights, class weights with one zero."""
    n = shape[-1] if len(shape) == 2 else shape[-2]
    tgt = torch.randint(0, N, shape, generator=g)
    tgt[torch.rand(shape, generator=g) < 0.1] = 255
    lab = torch.randint(0, N, shape, generator=g)
    conf = torch.rand(shape, generator=g)
    ign = torch.zeros(shape, dtype=torch.int64)
    ign[:, n // 3:n // 2] = 255
    mc = torch.randint(0, N, shape, generator=g)
    mc.view(B, -1)[:, ::2] = 255
    cw = torch.rand(N, generator=g) + 0.5
    cw[N // 2] = 0.0
    return tgt, lab, conf, ign, mc, torch.tensor([0.25, 0.75]), cw


def ce_cases(call, lg_shape, d, g, N, m_shape, out, key):
    """The four configurations of a fused cross entropy `call(dlogits=, gscale=, **kw)`: plain, confidence + guidance,
    img_weight + all_pixels, label smoothing + class weights (one weight zero); sums and gradient of each."""
    tgt, lab, conf, ign, mc, iw, cw = (t.to(d) for t in maps(g, N, m_shape))
    gs = torch.tensor([1.0 / tgt.numel(), 0.3 / tgt.numel()], device=d)
    cfgs = dict(plain=(tgt, True, {}),
                conf_guidance=(lab, False, dict(conf=conf, ign=ign, conf_thresh=0.7, mc=mc)),
                imgweight_allpixels=(lab, False, dict(conf=conf, ign=ign, conf_thresh=0.7, all_pixels=True, img_weight=iw)),
                lsw=(tgt, True, dict(label_smoothing=0.1, class_weight=cw)))
    for name, (t, use_ignore, kw) in cfgs.items():
        dl = torch.full(lg_shape, float("nan"), device=d)
        sums = call(t, use_ignore, dlogits=dl, gscale=gs, **kw)
        out[f"{key}/{name}/sums"], out[f"{key}/{name}/dlogits"] = sha(sums), sha(dl)
        out[f"{key}/{name}/sums_forward_only"] = sha(call(t, use_ignore, **kw))
    return tgt


def run(d):
    from semivl_amd import ops
    out = {}
    g = torch.Generator().manual_seed(20)
    for N, HW in FULL:
        key = f"full/N{N}_HW{HW}"
        lg = (torch.randn(B, N, HW, generator=g) * 3).to(d)
        conf, lab = ops.softmax_max(lg)
        out[key + "/softmax_max/conf"], out[key + "/softmax_max/label"] = sha(conf), sha(lab)
        tgt = ce_cases(lambda t, u, **kw: ops.ce_fused(lg, t, u, **kw), lg.shape, d, g, N, (B, HW), out, key + "/ce_fused")
        out[key + "/target_prob"] = sha(ops.target_prob(lg, tgt))
    for N, h, w, H, W in UP:
        for align in (False, True):
            key = f"up/N{N}_{h}x{w}_{H}x{W}_align{int(align)}"
            lg = (torch.randn(B, N, h, w, generator=g) * 3).to(d)
            conf, lab = ops.softmax_max_up(lg, H, W, align)
            out[key + "/softmax_max_up/conf"], out[key + "/softmax_max_up/label"] = sha(conf), sha(lab)
            tgt = ce_cases(lambda t, u, **kw: ops.ce_up_fused(lg, H, W, align, t, u, **kw), lg.shape, d, g, N, (B, H, W), out,
                           key + "/ce_up_fused")
            out[key + "/target_prob_up"] = sha(ops.target_prob(lg, tgt, up=(H, W, align)))
    for N, h, w, H, W in INDEX_ONLY:
        key = f"index/N{N}_{h}x{w}_{H}x{W}"
        x = torch.randn(B, N, h, w, generator=g).to(d)
        ign = maps(g, N, (B, H, W))[3].to(d)
        out[key + "/maskclip_labels"] = sha(ops.maskclip_labels(x, H, W, 10.0, 0.5, ign))
        out[key + "/tta_view"] = sha(ops.tta_view(x, H, W, False))
        out[key + "/tta_view_flip"] = sha(ops.tta_view(x, H, W, True))
        C = 8
        xr = torch.randn(B * h * w, C, generator=g).to(d)
        dyr = torch.randn(B * H * W, C, generator=g).to(d)
        dy = torch.randn(B, N, H, W, generator=g).to(d)
        base = torch.rand(B, N, H, W, generator=g).to(d)
        for align in (False, True):
            ka = f"{key}_align{int(align)}"
            out[ka + "/bilinear_planes_fwd"] = sha(ops.bilinear_planes_fwd(x, h, w, align, H, W))
            out[ka + "/bilinear_planes_bwd"] = sha(ops.bilinear_planes_bwd(dy, h, w, align, H, W))
            y = torch.full((B * H * W, C), float("nan"), device=d)
            ops.bilinear_nhwc_fwd(xr, C, B, h, w, C, align, 1, H, W, y, C)
            dx = torch.full((B * h * w, C), float("nan"), device=d)
            ops.bilinear_nhwc_bwd(dyr, C, B, h, w, C, align, 1, H, W, dx, C)
            out[ka + "/bilinear_nhwc_fwd"], out[ka + "/bilinear_nhwc_bwd"] = sha(y), sha(dx)
            for kind in (0, 1):
                src = x if kind == 0 else x.abs() + 0.1     # (kind 1: probability sums are positive)
                for flip in (False, True):
                    acc = ops.tta_accum(src, base.clone(), kind, align, flip, 0.5, True)
                    out[f"{ka}/tta_accum_kind{kind}_flip{int(flip)}"] = sha(acc)
    torch.cuda.synchronize()
    return out


def compare(pa, pb):
    a, b = (json.load(open(p))["digests"] for p in (pa, pb))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print("\n".join(f"{k}: differs" for k in bad) if bad else f"{len(a)} digests: equal bit for bit")
    return 1 if bad else 0


def main(run=run, tool="pixel_loss_digest"):
    """Command line of this tool and of the digest tools that import it (each with its own `run` and name)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                    help="the tree whose semivl_amd (and built library) to run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: needs the GPU")
    sys.path.insert(0, os.path.abspath(a.root))
    res = dict(tool=tool, device=torch.cuda.get_device_name(0), digests=run(torch.device("cuda:0")))
    print(f"{len(res['digests'])} digests")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
