"""svl_panel_image_u8 and svl_panel_label_u8 against the numpy restatement tests/panel_ref.py, byte for byte: there is no
tolerance.  Every run writes a tile into a strided canvas that lives inside a sentinel-filled buffer and the WHOLE buffer is
compared, so the guard bands around the tile and around the canvas are part of every check.  Shapes: one pixel, rows shorter
than a thread's 4 pixels, a multiple of everything, odd sizes whose groups run over row ends (65 x 63: H W is odd, the last
group of a sample is partial), and 2 x 512 x 512 = two trips of the capped grid (256 blocks x 256 threads x 4 pixels)."""
import numpy as np
import pytest
import torch

import panel_ref as P

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
SHAPES = [(1, 1), (3, 5), (64, 64), (65, 63)]


def make_canvas(B, H, W, dev, off=0, y0=2, x0=3, row_pad=7, batch_pad=5):
    """A canvas [B, y0 + H + 2, x0 + W + 1, 3] with padded row / batch strides at byte `off` of a sentinel buffer."""
    CH, CW = y0 + H + 2, x0 + W + 1
    rs = CW * 3 + row_pad
    bs = CH * rs + batch_pad
    buf = torch.full((32 + off + B * bs + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    canvas = torch.as_strided(buf, (B, CH, CW, 3), (bs, rs, 3, 1), 32 + off)
    return buf, canvas


def expect(buf_shape, canvas_like, tile, y0, x0, off):
    """The sentinel buffer with `tile` [B, H, W, 3] written at the tile's place."""
    B, H, W, _ = tile.shape
    bs, rs = canvas_like.stride(0), canvas_like.stride(1)
    want = np.full(buf_shape, SENTINEL, np.uint8)
    view = np.lib.stride_tricks.as_strided(want[32 + off:], (B, canvas_like.shape[1], canvas_like.shape[2], 3), (bs, rs, 3, 1))
    view[:, y0:y0 + H, x0:x0 + W] = tile
    return want


def check(kind, src, arg, dev, off=0, y0=2, x0=3, **kw):
    from semivl_amd import ops
    B, H, W = src.shape[0], src.shape[-2], src.shape[-1]
    buf, canvas = make_canvas(B, H, W, dev, off, y0, x0, **kw)
    if kind == "image":
        ops.panel_image(src, P.MEAN, P.STD, canvas, y0, x0)
        tile = P.image_tile(src.cpu().numpy())
    else:
        ops.panel_label(src, arg, canvas, y0, x0)
        tile = P.label_tile(src.cpu().numpy(), arg.cpu().numpy())
    want = torch.from_numpy(expect(tuple(buf.shape), canvas, tile, y0, x0, off)).to(dev)
    bad = (buf != want).nonzero().flatten()
    assert bad.numel() == 0, (kind, (B, H, W), off, bad[:8].tolist(), buf[bad[:8]].tolist(), want[bad[:8]].tolist())
    return buf


def images(B, H, W, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g) * 1.5
    flat = x.view(-1)
    for i, v in enumerate((float("nan"), float("inf"), float("-inf"), -7.0, 9.0, -2.1179039478302, 0.0)):
        flat[i::13] = v          # NaN, +-inf, v below 0 and above 1 (and a few on the grid)
    return x.to(dev)


def labels(B, H, W, K, seed, dev):
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, K, (B, H, W), generator=g)
    flat = m.view(-1)
    for i, v in enumerate((-1, K, 254, 255, 2 ** 40, K - 1, 0, -2 ** 40)):
        flat[i::17] = v
    return m.to(dev)


def palette(K, dev, seed=3):
    g = torch.Generator().manual_seed(seed + K)
    return torch.randint(0, 256, (K, 3), generator=g).to(torch.uint8).to(dev)


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_image_tiles(dev, B, hw):
    check("image", images(B, *hw, seed=B * 100 + hw[0], dev=dev), None, dev)


@pytest.mark.parametrize("K", [1, 21, 256])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_label_tiles(dev, B, hw, K):
    check("label", labels(B, *hw, K, seed=B * 100 + hw[1] + K, dev=dev), palette(K, dev), dev)


def test_two_trips_of_the_capped_grid(dev):
    """2 x 512 x 512 pixels: 131072 groups of 4 against a grid capped at 256 x 256 threads -- every block makes two trips."""
    check("image", images(2, 512, 512, 7, dev), None, dev, row_pad=0, batch_pad=0, x0=0, y0=0)
    check("label", labels(2, 512, 512, 21, 8, dev), palette(21, dev), dev, off=1)


@pytest.mark.parametrize("hw", [(3, 5), (8, 16), (65, 63)])
def test_every_byte_alignment_of_the_destination(dev, hw):
    """Tile origins at every byte alignment mod 16 (the buffer itself is 256-byte aligned): the 4-byte store path and the byte
    path, on rows whose alignment changes from row to row (odd row stride) and on rows that keep it (stride % 4 == 0)."""
    img, lab, pal = images(2, *hw, 11, dev), labels(2, *hw, 21, 12, dev), palette(21, dev)
    for off in range(16):
        for row_pad in (7, (4 - ((3 + hw[1] + 1) * 3) % 4) % 4):
            buf, canvas = make_canvas(2, *hw, dev, off, row_pad=row_pad)
            assert (canvas.data_ptr() + 2 * canvas.stride(1) + 9) % 16 == (off + 2 * canvas.stride(1) + 9) % 16
            check("image", img, None, dev, off=off, row_pad=row_pad)
            check("label", lab, pal, dev, off=off, row_pad=row_pad)


def test_rerun_is_bit_equal_and_tiles_do_not_touch_each_other(dev):
    from semivl_amd import ops
    B, H, W = 2, 33, 31
    img, lab, pal = images(B, H, W, 21, dev), labels(B, H, W, 21, 22, dev), palette(21, dev)
    runs = []
    for _ in range(2):
        canvas = torch.full((B, 2 * H, 2 * W, 3), SENTINEL, dtype=torch.uint8, device=dev)
        ops.panel_image(img, P.MEAN, P.STD, canvas, 0, 0)
        ops.panel_label(lab, pal, canvas, H, W)
        runs.append(canvas)
    assert torch.equal(runs[0], runs[1])
    got = runs[0].cpu().numpy()
    assert np.array_equal(got[:, :H, :W], P.image_tile(img.cpu().numpy()))
    assert np.array_equal(got[:, H:, W:], P.label_tile(lab.cpu().numpy(), pal.cpu().numpy()))
    assert (got[:, :H, W:] == SENTINEL).all() and (got[:, H:, :W] == SENTINEL).all()


@pytest.fixture(scope="module")
def edges():
    return [P.byte_edges(c) for c in range(3)]


def test_image_values_one_ulp_either_side_of_every_byte_crossing(dev, edges):
    """For each channel the inputs just below / at / just above the 255 points where v * 255 + 0.5 crosses an integer: a
    contracted multiply-add, or a rounding mode other than the restatement's, moves some of these bytes."""
    n = max(e.size for e in edges)
    assert min(e.size for e in edges) >= 4 * 250
    x = torch.zeros(1, 3, 1, n)
    for c, e in enumerate(edges):
        x[0, c, 0, :e.size] = torch.from_numpy(e)
    buf = check("image", x.to(dev), None, dev)
    tile = P.image_tile(x.numpy())[0, 0]
    for c, e in enumerate(edges):
        b = tile[:e.size, c].reshape(-1, 4).astype(np.int32)
        assert (b[:, 1] + 1 == b[:, 2]).all()          # the restatement itself steps exactly there
    assert buf.numel() > 0


def test_special_values(dev):
    x = torch.zeros(1, 3, 2, 8)
    x[0, :, 0] = torch.tensor([float("nan"), float("inf"), float("-inf"), -100.0, 100.0, 0.0, -2.2, 2.7])
    buf, canvas = make_canvas(1, 2, 8, dev)
    from semivl_amd import ops
    ops.panel_image(x.to(dev), P.MEAN, P.STD, canvas, 2, 3)
    row = canvas[0, 2, 3:11].cpu().numpy()
    assert row[:5].tolist() == [[0] * 3, [255] * 3, [0] * 3, [0] * 3, [255] * 3] and row[6].tolist() == [0] * 3 and row[7].tolist() == [255] * 3
    K = 21
    pal = palette(K, dev)
    lab = torch.tensor([[[-1, K, 254, 255, 2 ** 40, -2 ** 63, 2 ** 63 - 1, K - 1]]], dtype=torch.int64, device=dev)
    buf, canvas = make_canvas(1, 1, 8, dev)
    ops.panel_label(lab, pal, canvas, 2, 3)
    row = canvas[0, 2, 3:11].cpu().numpy()
    assert (row[:7] == 255).all() and row[7].tolist() == pal[K - 1].tolist()


def test_refusals_name_the_offender(dev):
    from semivl_amd import lib as L
    from semivl_amd import ops
    img, lab, pal = images(2, 4, 6, 1, dev), labels(2, 4, 6, 21, 2, dev), palette(21, dev)
    canvas = torch.zeros(2, 8, 12, 3, dtype=torch.uint8, device=dev)
    before = canvas.clone()
    for call, word in [
        (lambda: ops.panel_image(img[:, :2], P.MEAN, P.STD, canvas, 0, 0), r"\[B, 3, H, W\]"),
        (lambda: ops.panel_image(img.double(), P.MEAN, P.STD, canvas, 0, 0), "float32"),
        (lambda: ops.panel_image(img.cpu(), P.MEAN, P.STD, canvas, 0, 0), "GPU"),
        (lambda: ops.panel_image(img.transpose(2, 3), P.MEAN, P.STD, canvas, 0, 0), "contiguous"),
        (lambda: ops.panel_image(img, P.MEAN[:2], P.STD, canvas, 0, 0), "mean and std"),
        (lambda: ops.panel_image(img, P.MEAN, P.STD, canvas.int(), 0, 0), "canvas"),
        (lambda: ops.panel_image(img, P.MEAN, P.STD, canvas[..., :2], 0, 0), "canvas"),
        (lambda: ops.panel_image(img, P.MEAN, P.STD, canvas.permute(0, 2, 1, 3), 0, 0), "canvas"),
        (lambda: ops.panel_image(img, P.MEAN, P.STD, canvas[:1], 0, 0), "holds 1 samples"),
        (lambda: ops.panel_image(img, P.MEAN, P.STD, canvas, 5, 0), "does not lie inside"),
        (lambda: ops.panel_image(img, P.MEAN, P.STD, canvas, 0, 7), "does not lie inside"),
        (lambda: ops.panel_image(img, P.MEAN, P.STD, canvas, -1, 0), "does not lie inside"),
        (lambda: ops.panel_image(img, P.MEAN, P.STD, canvas, 0.0, 0), "y0 must be an int"),
        (lambda: ops.panel_image(img, P.MEAN, P.STD, canvas, 0, True), "x0 must be an int"),
        (lambda: ops.panel_label(lab.int(), pal, canvas, 0, 0), "int64"),
        (lambda: ops.panel_label(lab[0], pal, canvas, 0, 0), r"\[B, H, W\]"),
        (lambda: ops.panel_label(lab, pal.view(-1), canvas, 0, 0), "palette"),
        (lambda: ops.panel_label(lab, pal.int(), canvas, 0, 0), "palette"),
        (lambda: ops.panel_label(lab, pal.cpu(), canvas, 0, 0), "palette"),
        (lambda: ops.panel_label(lab, pal[:0], canvas, 0, 0), "palette"),
        (lambda: ops.panel_label(lab, torch.zeros(257, 3, dtype=torch.uint8, device=dev), canvas, 0, 0), "palette"),
        (lambda: ops.panel_label(lab, pal, canvas, 4, 7), "does not lie inside"),
    ]:
        with pytest.raises(ValueError, match=word):
            call()
    # the C entry points' own refusals
    lib = L.load()
    m3, s3 = (L.C.c_float * 3)(*P.MEAN.tolist()), (L.C.c_float * 3)(*P.STD.tolist())
    ip, lp, pp, cp = img.data_ptr(), lab.data_ptr(), pal.data_ptr(), canvas.data_ptr()
    bs, rs = canvas.stride(0), canvas.stride(1)
    for args, word in [((None, 2, 4, 6, m3, s3, cp, bs, rs), "null"), ((ip, 2, 4, 6, m3, s3, None, bs, rs), "null"),
                       ((ip, 2, 4, 6, None, s3, cp, bs, rs), "mean3"), ((ip, 0, 4, 6, m3, s3, cp, bs, rs), "B = 0"),
                       ((ip, 2, 0, 6, m3, s3, cp, bs, rs), "H = 0"), ((ip, 2, 4, -1, m3, s3, cp, bs, rs), "W = -1"),
                       ((ip, 2, 4, 6, m3, s3, cp, bs, 17), "row_stride"), ((ip, 2, 4, 6, m3, s3, cp, 3 * rs + 17, rs), "batch_stride"),
                       ((ip + 2, 2, 4, 6, m3, s3, cp, bs, rs), "4-byte aligned"),
                       ((ip, 2 ** 15, 2 ** 8, 2 ** 8, m3, s3, cp, 2 ** 40, 2 ** 20), "32-bit index")]:
        assert lib.svl_panel_image_u8(*args, None) == -1 and word in L.last_error() and "svl_panel_image_u8" in L.last_error(), L.last_error()
    for args, word in [((None, 2, 4, 6, pp, 21, cp, bs, rs), "null"), ((lp, 2, 4, 6, None, 21, cp, bs, rs), "palette"),
                       ((lp, 2, 4, 6, pp, 0, cp, bs, rs), "K = 0"), ((lp, 2, 4, 6, pp, 257, cp, bs, rs), "K = 257"),
                       ((lp, 2, 4, 0, pp, 21, cp, bs, rs), "W = 0"), ((lp, 2, 4, 6, pp, 21, cp, bs, 3 * 6 - 1), "row_stride"),
                       ((lp, 2, 4, 6, pp, 21, cp, 0, rs), "batch_stride"), ((lp + 4, 2, 4, 6, pp, 21, cp, bs, rs), "8-byte aligned")]:
        assert lib.svl_panel_label_u8(*args, None) == -1 and word in L.last_error() and "svl_panel_label_u8" in L.last_error(), L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(canvas, before)
