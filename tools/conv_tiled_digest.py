"""What the tiled 3x3 convolutions of csrc/conv_tiled.hip and the dilated whole-image kernel of csrc/conv_dil.hip (which shares
the split helpers of csrc/planes_split.h with them) compute, bit for bit, to compare two builds of the library: seeded
CPU-generated inputs on the shapes of the tiled-convolution cases of tests/test_ops_gpu.py (the walking-tiles shapes included),
forward / input gradient / both GroupNorm epilogues / weight planes / weight gradient in modes 0 and 6, with the planes image
and with a bare pack, every output NaN-prefilled (an element a kernel leaves unwritten shows), and one SHA-256 per (entry,
shape, variant) over the outputs written to a JSON file.  One build per process; command line, `sha` and `compare` are
tools/pixel_loss_digest.py's.
usage: python tools/conv_tiled_digest.py [--root TREE] --out FILE.json
       python tools/conv_tiled_digest.py --compare A.json B.json"""
import hashlib
import sys

import torch

from pixel_loss_digest import main, sha

# (C1, C2, Co, H, W, n, rep): the cases of test_conv3x3_with_groupnorm_statistics / test_conv3x3_presplit_weight_planes /
# test_tiled_narrow_conv3x3_split_emulation (every split instantiation, ragged patches, two concat sources)
SHAPES = [(64, 0, 64, 32, 32, 16, 1), (96, 32, 64, 16, 48, 24, 3), (64, 0, 32, 40, 24, 18, 1), (32, 0, 32, 64, 64, 4, 1),
          (48, 16, 32, 16, 16, 66, 2), (32, 0, 32, 19, 37, 24, 1), (16, 16, 32, 19, 37, 24, 8), (32, 0, 32, 61, 70, 5, 1)]
# (C, Co, H, W) of test_tiled_conv3x3_blocks_walk_several_tiles: the image count follows from the CU count
WALK = [(32, 64, 8, 16), (16, 32, 16, 16), (16, 32, 9, 17)]
# (Ct, Co, H, W, n) of the weight gradient: the three split kernels (<2, 1>, <1, 2>, <1, 1, 2>), Co = 128, and Ct = 32 -> Co = 64
WGRAD = [(32, 64, 32, 32, 16), (64, 32, 32, 32, 16), (32, 32, 32, 64, 8), (64, 128, 24, 40, 18), (96, 32, 19, 37, 24)]
DIL = [(9, 6), (17, 12), (8, 18)]          # (images, dilation) of the 128 -> 128 convolutions on 32 x 32 maps


def run(d):
    from semivl_amd import ops, lib as L
    lib, p, st = L.load(), ops._p, ops._st
    out = {}
    g = torch.Generator().manual_seed(44)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(d)

    def nans(*shape, dtype=torch.float32):
        return torch.full(shape, float("nan"), dtype=dtype, device=d)

    def put(key, **tensors):
        h = hashlib.sha256()
        for n, t in tensors.items():
            h.update(f"{n}={sha(t)};".encode())
        assert key not in out, key
        out[key] = h.hexdigest()

    def packs(w):
        wf, wd = ops.pack_conv_w(w)
        return {"planes": (wf, wd), "bare": (wf.clone(), wd.clone())}

    def conv_cases(tag, x, C1, n, H, W, Co, w, kw, x2=None):
        """Forward with every epilogue, forward + GroupNorm statistics (with and without gn_in), input gradient plain /
        accumulated / with the GroupNorm-backward sums: modes 0 and 6, planes and bare."""
        Ct = w.shape[1]
        bias, dy, base = rnd(Co), rnd(n * H * W, Co), rnd(n * H * W, Ct)
        table = torch.stack([rnd(n, C1) * 0.2 + 1.0, rnd(n, C1) * 0.2], 1).contiguous()      # gn_in [n, 2, C1]
        gn_x, gamma, beta = rnd(n * H * W, Ct), rnd(Ct) + 1.0, rnd(Ct)
        G = Ct // 16
        stx = ops.groupnorm_fwd(gn_x, Ct, gamma, beta, 1e-5, n, H * W, Ct, G, True, ops.empty(n * H * W, Ct, device=d), Ct)
        gtab = ops.groupnorm_scale_shift(stx, gamma, beta, n, Ct, G)
        for mode in (0, 6):
            ops.set_gemm_emulation(mode)
            for name, (wf, wd) in packs(w).items():
                key = f"{tag}/mode{mode}_{name}"
                for ep, ekw in (("plain", {}), ("bias_relu", dict(bias=bias, act=ops.ACT_RELU)), ("gelu", dict(act=ops.ACT_GELU))):
                    y = nans(n * H * W, Co)
                    ops.conv_fwd(x, C1, n, H, W, C1, wf, Co, 3, 3, 1, 1, out=y, ldo=Co, **ekw, **kw)
                    put(f"conv_fwd/{key}/{ep}", y=y, path=torch.tensor(lib.svl_last_gemm_path()))
                for gi in (None, table):
                    ws = nans(max(1, lib.svl_conv3x3_gn_ws_doubles(n, H, W, Co)), dtype=torch.float64)
                    pre, stats = nans(n * H * W, Co), nans(n, Co // 16, 2)
                    rc = lib.svl_conv3x3_gn_f32(p(x), C1, C1, p(x2), kw.get("ld2", 0), kw.get("C2", 0), kw.get("rep", 1), p(wf), n, H, W, Co,
                                                p(pre), Co, 1e-5, p(ws), p(stats), p(gi), p(ops.w_planes_of(wf)), st())
                    put(f"conv3x3_gn/{key}/gn_in{int(gi is not None)}", rc=torch.tensor(rc), pre=pre, stats=stats, ws=ws)
                if Ct in (32, 64):                       # the input gradient is a narrow convolution too
                    dx = nans(n * H * W, Ct)
                    ops.conv_dgrad(dy, Co, n, H, W, Co, wd, Ct, 3, 3, 1, 1, out=dx, ldo=Ct)
                    acc = base.clone()
                    ops.conv_dgrad(dy, Co, n, H, W, Co, wd, Ct, 3, 3, 1, 1, out=acc, ldo=Ct, accumulate=True)
                    put(f"conv_dgrad/{key}", dx=dx, acc=acc, path=torch.tensor(lib.svl_last_gemm_path()))
                    for accumulate in (0, 1):
                        ws = nans(max(1, lib.svl_conv3x3_gnb_ws_doubles(n, H, W, Ct)), dtype=torch.float64)
                        o, cs = (base.clone() if accumulate else nans(n * H * W, Ct)), nans(n, 2, Ct)
                        rc = lib.svl_conv3x3_dgrad_gnb_f32(p(dy), Co, Co, p(wd), n, H, W, Ct, p(o), Ct, accumulate, p(gn_x), p(gtab), p(stx),
                                                           p(ws), p(cs), p(ops.w_planes_of(wd)), st())
                        put(f"conv3x3_dgrad_gnb/{key}/acc{accumulate}", rc=torch.tensor(rc), dx=o, chan_sums=cs, ws=ws)
            if mode == 6:
                for which, pk in zip(("fwd", "dgrad"), packs(w)["planes"]):
                    if ops.w_planes_of(pk) is not None:
                        N_, K_ = pk.shape
                        img = torch.full((lib.svl_conv3x3_weight_planes_bytes(N_, K_ // 9),), 0xA5, dtype=torch.uint8, device=d)
                        L.check(lib.svl_conv3x3_weight_planes(p(pk), N_, K_ // 9, p(img), st()), "weight planes")
                        put(f"weight_planes/{tag}/{which}", image=img)

    for C1, C2, Co, H, W, n, rep in SHAPES:
        x = rnd(n * H * W, C1)
        x2 = rnd(n // rep * H * W, C2) if C2 else None
        w = rnd(Co, C1 + C2, 3, 3, scale=0.1)
        if (C1, C2, Co) == (64, 0, 64):
            w[5] = 0.0                                  # an all-zero output channel: exponent 0 in the planes image
        kw = dict(src2=x2, ld2=C2, C2=C2, rep=rep) if C2 else {}
        conv_cases(f"C{C1}+{C2}_Co{Co}_{H}x{W}_n{n}_rep{rep}", x, C1, n, H, W, Co, w, kw, x2)

    cus = torch.cuda.get_device_properties(d).multi_processor_count
    for C, Co, H, W in WALK:
        per_img = -(-H // (16 if Co == 32 and H >= 16 else 8)) * -(-W // 16)
        n = -(-(4 * cus + 3) // per_img)
        scale = torch.tensor([2.0 ** (3 * ((5 * i) % 7) - 9) for i in range(n)]).view(n, 1, 1, 1)
        x = torch.randint(-4, 5, (n, H, W, C), generator=g).float() * scale
        x[n // 2] = 0.0
        w = (torch.randint(-4, 5, (Co, C, 3, 3), generator=g).float() / 8).to(d)
        xs = x.view(-1, C).to(d)
        conv_cases(f"walk/C{C}_Co{Co}_{H}x{W}_n{n}", xs, C, n, H, W, Co, w, {})
        # the mirrored-tap form at the same instantiation: input gradient of a convolution Co -> C, Co outputs
        wb = (torch.randint(-4, 5, (C, Co, 3, 3), generator=g).float() / 8).to(d)
        ops.set_gemm_emulation(6)
        for name, (_, wd) in packs(wb).items():
            dx = nans(n * H * W, Co)
            ops.conv_dgrad(xs, C, n, H, W, C, wd, Co, 3, 3, 1, 1, out=dx, ldo=Co)
            put(f"conv_dgrad_mirrored/walk/C{C}_Co{Co}_{H}x{W}_n{n}/mode6_{name}", dx=dx, path=torch.tensor(lib.svl_last_gemm_path()))

    for Ct, Co, H, W, n in WGRAD:
        x, dy = rnd(n * H * W, Ct), rnd(n * H * W, Co)
        x[: H * W] *= 2.0 ** 12                          # (the running exponents of the split kernel move)
        table = torch.stack([rnd(n, Ct) * 0.2 + 1.0, rnd(n, Ct) * 0.2], 1).contiguous()
        for mode in (0, 6):
            ops.set_gemm_emulation(mode)
            if Co == 128 and mode == 0:
                continue
            groups = lib.svl_conv3x3_wgrad_tiled_groups(n, H, W, Ct, Co)
            for gi in (None, table):
                slabs = nans(groups, Co, 9 * Ct)
                L.check(lib.svl_conv3x3_wgrad_tiled(p(dy), Co, Co, p(x), Ct, Ct, None, 0, 0, 1, n, H, W, p(slabs), groups, p(gi), st()), "wgrad")
                put(f"conv_wgrad/Ct{Ct}_Co{Co}_{H}x{W}_n{n}/mode{mode}_gn_in{int(gi is not None)}", slabs=slabs,
                    groups=torch.tensor(groups), path=torch.tensor(lib.svl_last_gemm_path()))
    # two concat sources with class repetition (a slab that straddles them)
    n, H, W, C1, C2, Co, rep = 24, 16, 48, 96, 32, 64, 3
    x, x2, dy = rnd(n * H * W, C1), rnd(n // rep * H * W, C2), rnd(n * H * W, Co)
    for mode in (0, 6):
        ops.set_gemm_emulation(mode)
        groups = lib.svl_conv3x3_wgrad_tiled_groups(n, H, W, C1 + C2, Co)
        slabs = nans(groups, Co, 9 * (C1 + C2))
        L.check(lib.svl_conv3x3_wgrad_tiled(p(dy), Co, Co, p(x), C1, C1, p(x2), C2, C2, rep, n, H, W, p(slabs), groups, None, st()), "wgrad")
        put(f"conv_wgrad/C{C1}+{C2}_Co{Co}_{H}x{W}_n{n}_rep{rep}/mode{mode}", slabs=slabs)

    ops.set_gemm_emulation(6)
    C = 128
    w = rnd(C, C, 3, 3, scale=0.1)
    wf, wd = ops.pack_conv_w(w)
    for n, dil in DIL:
        x, dy, base = rnd(n * 1024, C), rnd(n * 1024, C), rnd(n * 1024, C)
        x[:1024] *= 2.0 ** -30
        x[:, 16:] *= 2.0 ** 10                           # (the tile's exponent is outgrown: the flush path)
        y, dx, acc = nans(n * 1024, C), nans(n * 1024, C), base.clone()
        ops.conv_fwd(x, C, n, 32, 32, C, wf, C, 3, 3, dil, dil, out=y, ldo=C)
        path = lib.svl_last_gemm_path()
        ops.conv_dgrad(dy, C, n, 32, 32, C, wd, C, 3, 3, dil, dil, out=dx, ldo=C)
        ops.conv_dgrad(dy, C, n, 32, 32, C, wd, C, 3, 3, dil, dil, out=acc, ldo=C, accumulate=True)
        put(f"conv_dil/n{n}_d{dil}", y=y, dx=dx, acc=acc, path=torch.tensor(path))
    ops.set_gemm_emulation(0)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    sys.exit(main(run, "conv_tiled_digest"))
