"""Golden vectors for the debug panels (svl_panel_image_u8 / svl_panel_label_u8, tests/panel_ref.py): label maps up to
24 x 20 that contain -1, 0, K-1, K, 254 and 255, the output of the reference's OWN colorize_label
(utils/plot_utils.py:21-26) on each with the reference's get_palette('pascal') (datasets/palettes.py, recorded as data:
256 entries, K = 256) and with its first 21 entries alone (K = 21: 254 and 255 are then outside the palette),
and the fp32 result of plot_data's `data.permute([1, 2, 0]).mul(std).add(mean)` (plot_utils.py:32-34) for a small image.
Runs only where the reference tree exists: `python gen_golden_panel.py <path to the reference tree>`.  Writes
tests/golden/panel_cases.npz (a few KB).

plot_utils.py imports matplotlib at module level and only plot_data's drawing calls use it; where matplotlib is not
installed an empty stand-in module is registered for the import."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {"a": (24, 20), "b": (7, 13), "c": (1, 1)}


def load(ref, name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def label_map(name, K):
    h, w = SHAPES[name]
    rng = np.random.RandomState(sorted(SHAPES).index(name) + 71)
    m = rng.randint(0, K, (h, w)).astype(np.int64)
    for i, v in enumerate((-1, 0, K - 1, K, 254, 255)):
        m.reshape(-1)[i::11] = v
    return m


def main():
    ref = os.path.abspath(sys.argv[1])
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot
    plot = load(ref, "_ref_plot_utils", "utils", "plot_utils.py")
    pal = load(ref, "_ref_palettes", "datasets", "palettes.py")
    palette = np.asarray(pal.get_palette("pascal")).astype(np.uint8).reshape(-1, 3)
    K = len(palette)
    out = {"names": np.array(sorted(SHAPES)), "pascal_palette": palette}
    for name in sorted(SHAPES):
        for tag, k in (("", K), ("21", 21)):       # the whole recorded palette, and its 21 class colours alone
            m = label_map(name, k)
            out[f"{name}/label{tag}"] = m
            out[f"{name}/color{tag}"] = plot.colorize_label(m, palette[:k])
            print(name, k, m.shape, "white pixels", int((out[f"{name}/color{tag}"] == 255).all(-1).sum()))
    rng = np.random.RandomState(5)
    img = (rng.randn(3, 9, 11) * 1.3).astype(np.float32)
    img[0, 0, :4] = [np.nan, np.inf, -np.inf, 0.0]
    shown = []
    ax = types.SimpleNamespace(imshow=shown.append, axis=lambda *_: None, set_title=lambda *_: None)
    plot.plot_data(ax, None, "image", torch.from_numpy(img))        # the reference's own mean / std and operations
    out["image"] = img
    out["image_float"] = shown[0].numpy()
    # ... and its 'label' branch agrees with colorize_label called directly
    plot.plot_data(ax, None, "label", torch.from_numpy(out["a/label"])[None], palette=palette)
    assert np.array_equal(shown[1], out["a/color"])
    path = os.path.join(HERE, "panel_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote panel_cases.npz", os.path.getsize(path), "bytes,", K, "palette entries")


if __name__ == "__main__":
    main()
