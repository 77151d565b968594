"""Golden vectors for the pseudo-label meter's table (svl_pl_stats_i64): a handful of 2 x 24 x 20 label-map cases, N in
{1, 2, 21}, with the three (intersection, union, target) triples of the reference's OWN intersectionAndUnion
(third_party/unimatch/util/utils.py:91-103) on the masked targets -- the pseudo-labels against the annotation where it
exists on a valid pixel, the confident pseudo-labels where the pixel is confident too, the guidance where it speaks.
Runs only where the reference tree exists: `python gen_golden_plstats.py <path to the reference tree>`.  Writes
tests/golden/plstats_cases.npz (inputs + triples; a few KB)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (N, bins, thresh, with mc, with gt)
CASES = {"n1": (1, 20, 0.95, True, True), "n2": (2, 1, 0.5, True, True), "voc": (21, 20, 0.95, True, True),
         "voc_nomc": (21, 20, 0.95, False, True), "voc_edges": (21, 7, 0.75, True, True)}
SHAPE = (2, 24, 20)


def blocks(rng, N, cell=4):
    """A piecewise-constant label map: one class per cell x cell block."""
    small = rng.randint(0, N, (SHAPE[0], SHAPE[1] // cell, SHAPE[2] // cell))
    return np.repeat(np.repeat(small, cell, 1), cell, 2).astype(np.int64)


def make_case(name):
    N, bins, thresh, with_mc, with_gt = CASES[name]
    rng = np.random.RandomState(sorted(CASES).index(name) + 11)
    gt = blocks(rng, N)
    p = np.where(rng.rand(*SHAPE) < 0.7, gt, rng.randint(0, N, SHAPE)).astype(np.int64)      # mostly right
    conf = rng.rand(*SHAPE).astype(np.float32) ** 0.25                                        # skewed towards 1
    ign = np.zeros(SHAPE, np.int64)
    ign[:, -3:, :] = 255
    ign[1, :, -4:] = 255                                                                     # padding: bottom and right
    mc = np.where(rng.rand(*SHAPE) < 0.5, np.where(rng.rand(*SHAPE) < 0.6, gt, rng.randint(0, N, SHAPE)), 255).astype(np.int64)
    mc[ign == 255] = 255                                                                     # semivl.py:239-240
    gt = gt.copy()
    gt[rng.rand(*SHAPE) < 0.05] = 255                                                        # void
    gt[ign == 255] = 254                                                                     # the loader's padding value
    if name == "voc_edges":
        p.reshape(-1)[::17] = -1
        p.reshape(-1)[5::23] = 255
        conf.reshape(-1)[::5] = np.float32(thresh)
        conf.reshape(-1)[1::7] = 1.0
        conf.reshape(-1)[2::11] = 0.0
        conf.reshape(-1)[3::13] = np.nan
        mc[0, :4, :] = 7                                                                     # guidance on a block, also where gt is void
        gt[1, 2:6, 2:9] = 254                                                                # padding value inside the valid area
    return dict(N=N, bins=bins, thresh=thresh, mask_w=p, conf=conf, ign=ign, mc=mc if with_mc else None,
                gt=gt if with_gt else None)


def main():
    ref = os.path.abspath(sys.argv[1])
    os.chdir(ref)
    sys.path.insert(0, ref)
    sys.path.insert(0, HERE)
    import _ref_shim
    _ref_shim.install()
    from third_party.unimatch.util.utils import intersectionAndUnion as ref_iau
    out = {"names": np.array(sorted(CASES))}
    for name in sorted(CASES):
        c = make_case(name)
        N, p, gt, mc = c["N"], c["mask_w"], c["gt"], c["mc"]
        for k_ in ("mask_w", "conf", "ign", "mc", "gt"):
            if c[k_] is not None:
                out[f"{name}/{k_}"] = c[k_]
        out[f"{name}/cfg"] = np.array([N, c["bins"]], np.int64)
        out[f"{name}/thresh"] = np.array(c["thresh"], np.float32)
        v = c["ign"] != 255
        with np.errstate(invalid="ignore"):
            k = v & (c["conf"] >= np.float32(c["thresh"]))
        g = v & (gt >= 0) & (gt < N)
        m = v & (mc >= 0) & (mc < N) if mc is not None else np.zeros_like(v)
        for tag, pred, cond in (("pl", p, g), ("plc", p, k & g), ("mc", mc if mc is not None else p, m & g)):
            target = np.where(cond, gt, 255)
            inter, union, tgt = ref_iau(pred, target, N, 255)
            out[f"{name}/{tag}_iut"] = np.stack([inter, union, tgt]).astype(np.int64)
        print(name, "pl inter", int(out[f"{name}/pl_iut"][0].sum()), "plc", int(out[f"{name}/plc_iut"][0].sum()),
              "mc", int(out[f"{name}/mc_iut"][0].sum()))
    path = os.path.join(HERE, "plstats_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote plstats_cases.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
