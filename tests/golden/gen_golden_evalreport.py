"""Golden vectors for the evaluation report's confusion table (svl_confusion_i64): 2 x 24 x 20 label maps, K in {1, 2, 21},
with targets 255 (ignored), 254 and -1 (neither a class nor ignored) and predictions -1 / 255 present, and the
(intersection, union, target) triple of the reference's OWN intersectionAndUnion
(third_party/unimatch/util/utils.py:91-103) on each; plus the reference's get_palette('pascal') (datasets/palettes.py) as
data.  Runs only where the reference tree exists: `python gen_golden_evalreport.py <path to the reference tree>`.  Writes
tests/golden/evalreport_cases.npz (inputs + triples + the palette; a few KB).

(No label equals K itself: np.histogram's last bin is closed, so the reference counts a label K as class K - 1.)"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {"k1": 1, "k2": 2, "voc": 21, "voc_edges": 21}
SHAPE = (2, 24, 20)


def blocks(rng, K, cell=4):
    """A piecewise-constant label map: one class per cell x cell block."""
    small = rng.randint(0, K, (SHAPE[0], SHAPE[1] // cell, SHAPE[2] // cell))
    return np.repeat(np.repeat(small, cell, 1), cell, 2).astype(np.int64)


def make_case(name):
    K = CASES[name]
    rng = np.random.RandomState(sorted(CASES).index(name) + 31)
    target = blocks(rng, K)
    pred = np.where(rng.rand(*SHAPE) < 0.7, target, rng.randint(0, K, SHAPE)).astype(np.int64)      # mostly right
    target = target.copy()
    target[rng.rand(*SHAPE) < 0.06] = 255                                                          # void
    target[:, -3:, :] = 255                                                                        # padding, ignored
    target[1, 2:6, 2:9] = 254                                                                      # the loader's padding value
    target.reshape(-1)[3::41] = -1
    if name == "voc_edges":
        pred.reshape(-1)[::17] = -1
        pred.reshape(-1)[5::23] = 255
        pred.reshape(-1)[7::29] = 254
    return K, pred, target


def main():
    ref = os.path.abspath(sys.argv[1])
    os.chdir(ref)
    sys.path.insert(0, ref)
    sys.path.insert(0, HERE)
    import _ref_shim
    _ref_shim.install()
    from third_party.unimatch.util.utils import intersectionAndUnion as ref_iau
    spec = importlib.util.spec_from_file_location("_ref_palettes", os.path.join(ref, "datasets", "palettes.py"))
    pal = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pal)
    out = {"names": np.array(sorted(CASES)),
           "pascal_palette": np.asarray(pal.get_palette("pascal")).astype(np.uint8).reshape(-1, 3)}
    for name in sorted(CASES):
        K, pred, target = make_case(name)
        inter, union, tgt = ref_iau(pred, target, K, 255)
        out[f"{name}/K"] = np.array(K, np.int64)
        out[f"{name}/pred"], out[f"{name}/target"] = pred, target
        out[f"{name}/iut"] = np.stack([inter, union, tgt]).astype(np.int64)
        print(name, "K", K, "inter", int(inter.sum()), "union", int(union.sum()), "target", int(tgt.sum()))
    path = os.path.join(HERE, "evalreport_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote evalreport_cases.npz", os.path.getsize(path), "bytes,", len(out["pascal_palette"]), "palette entries")


if __name__ == "__main__":
    main()
