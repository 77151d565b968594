"""tests/panel_ref.py (the numpy restatement the panel kernels are compared with) against tests/golden/panel_cases.npz, the
recorded output of the reference's own utils/plot_utils.py: colours equal, the float stage of the image rule bit-equal."""
import os

import numpy as np
import pytest

import panel_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "panel_cases.npz"))


@pytest.mark.parametrize("name", ["a", "b", "c"])
@pytest.mark.parametrize("tag,K", [("", 256), ("21", 21)])
def test_label_tile_is_colorize_label(golden, name, tag, K):
    label, want = golden[f"{name}/label{tag}"], golden[f"{name}/color{tag}"]
    pal = golden["pascal_palette"][:K]
    present = set(label.reshape(-1).tolist())
    if label.size >= 6:
        assert {-1, 0, K - 1, K, 254, 255} <= present
    got = P.label_tile(label, pal)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert (got[(label < 0) | (label >= K)] == 255).all()


def test_recorded_palette_is_the_voc_colour_map_on_the_classes(golden):
    from semivl_amd.report import voc_palette
    pal = golden["pascal_palette"]
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    voc = np.array(voc_palette(256), np.uint8).reshape(-1, 3)
    assert np.array_equal(pal[:21], voc[:21]) and np.array_equal(pal[255], voc[255])


def test_image_float_stage_is_bit_equal(golden):
    img, want = golden["image"], golden["image_float"]
    got = P.image_float(img)
    assert got.dtype == np.float32 and got.shape == want.shape == (9, 11, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(want[0, 0, 0]) and np.isposinf(want[0, 1, 0]) and np.isneginf(want[0, 2, 0])
    # ... and it is not the contracted form: a fused multiply-add differs from it somewhere on this image
    fused = (img.astype(np.float64).transpose(1, 2, 0) * P.STD.astype(np.float64) + P.MEAN.astype(np.float64)).astype(np.float32)
    ok = np.isfinite(want)
    assert (fused[ok] != want[ok]).any()


def test_image_tile_rule():
    x = np.zeros((3, 1, 6), np.float32)
    x[0, 0] = [np.nan, np.inf, -np.inf, -5.0, 5.0, 0.0]
    t = P.image_tile(x)
    assert t.dtype == np.uint8 and t[0, :, 0].tolist() == [0, 255, 0, 0, 255, int(np.float32(0.485) * np.float32(255) + np.float32(0.5))]
    # monotone, and every byte is reached
    xs = np.linspace(-2.2, 2.7, 20001, dtype=np.float32)
    img = np.broadcast_to(xs, (3, 1, xs.size)).copy()
    b = P.image_tile(img)[0]
    assert (np.diff(b.astype(np.int32), axis=0) >= 0).all()
    for c in range(3):
        assert set(b[:, c].tolist()) == set(range(256))


def test_byte_edges_sit_on_the_crossings():
    for c in range(3):
        xs = P.byte_edges(c, 100, 110)
        assert xs.size == 4 * 10
        img = np.zeros((3, 1, xs.size), np.float32)
        img[c, 0] = xs
        b = P.image_tile(img)[0, :, c].reshape(-1, 4).astype(np.int32)
        assert (b[:, 1] + 1 == b[:, 2]).all() and (b[:, 0] <= b[:, 1]).all() and (b[:, 2] <= b[:, 3]).all()
        assert b[:, 2].tolist() == list(range(101, 111))


def test_canvas_layout():
    rng = np.random.RandomState(0)
    B, H, W = 2, 3, 5
    imgs = [rng.randn(B, 3, H, W).astype(np.float32) for _ in range(4)]
    maps = [[rng.randint(-1, 5, (B, H, W)).astype(np.int64) for _ in range(4)] for _ in range(3)]
    maps[2][0] = None
    pal = rng.randint(0, 255, (4, 3)).astype(np.uint8)
    c4, c3 = P.canvas(imgs, maps, pal), P.canvas(imgs, maps[:2], pal)
    assert c4.shape == (B, 4 * H, 4 * W, 3) and c3.shape == (B, 3 * H, 4 * W, 3) and np.array_equal(c4[:, :3 * H], c3)
    assert np.array_equal(c4[:, :H, 2 * W:3 * W], P.image_tile(imgs[2]))
    assert np.array_equal(c4[:, 2 * H:3 * H, 3 * W:], P.label_tile(maps[1][3], pal))
    assert (c4[:, 3 * H:, :W] == 255).all()
