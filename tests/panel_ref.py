"""numpy restatement of the debug panels (semivl_amd/panel.py, svl_panel_image_u8 / svl_panel_label_u8): the two tile rules
and the canvas layout.  Exact: bytes are compared with ==, the float stage of the image rule bit for bit.

  image tile   v = x * std[c] + mean[c] as two fp32 operations (torch's permute.mul(std).add(mean), plot_utils.py:32-34),
               clamp to [0, 1] with NaN -> 0 (what imshow shows of a float image), byte = uint8(v * 255 + 0.5) in fp32
  label tile   palette[l] for 0 <= l < K, white otherwise (plot_utils.py:21-26, colorize_label)
  canvas       uint8 [B, rows * H, 4 * W, 3]: the images, then rows of label tiles, None = a white tile
"""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def image_float(img, mean=MEAN, std=STD):
    """img fp32 [..., 3, H, W] -> fp32 [..., H, W, 3]: x * std + mean, each operation rounded to fp32."""
    x = np.moveaxis(np.asarray(img, np.float32), -3, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x * np.asarray(std, np.float32)).astype(np.float32)
        return (t + np.asarray(mean, np.float32)).astype(np.float32)


def image_tile(img, mean=MEAN, std=STD):
    """-> uint8 [..., H, W, 3]."""
    v = image_float(img, mean, std)
    v = np.where(v > 0, v, np.float32(0))          # NaN and everything <= 0
    v = np.where(v < 1, v, np.float32(1)).astype(np.float32)
    u = (v * np.float32(255.0)).astype(np.float32)
    return (u + np.float32(0.5)).astype(np.float32).astype(np.uint8)     # 0.5 .. 255.5: truncation


def label_tile(label, palette):
    """label int64 [..., H, W], palette uint8 [K, 3] -> uint8 [..., H, W, 3]."""
    label, palette = np.asarray(label, np.int64), np.asarray(palette, np.uint8).reshape(-1, 3)
    K = palette.shape[0]
    ok = (label >= 0) & (label < K)
    out = np.full(label.shape + (3,), 255, np.uint8)
    out[ok] = palette[label[ok]]
    return out


def canvas(images, label_rows, palette, mean=MEAN, std=STD):
    """images: 4 arrays [B, 3, H, W]; label_rows: rows of 4 arrays [B, H, W] or None -> uint8 [B, rows * H, 4 * W, 3]."""
    B, _, H, W = images[0].shape
    out = np.zeros((B, (1 + len(label_rows)) * H, 4 * W, 3), np.uint8)
    for j, img in enumerate(images):
        out[:, :H, j * W:(j + 1) * W] = image_tile(img, mean, std)
    for i, row in enumerate(label_rows):
        for j, m in enumerate(row):
            tile = np.full((B, H, W, 3), 255, np.uint8) if m is None else label_tile(m, palette)
            out[:, (1 + i) * H:(2 + i) * H, j * W:(j + 1) * W] = tile
    return out


def byte_edges(c, lo=0, hi=255):
    """For channel c: normalised inputs x whose v = x * std + mean sits one ulp either side of the points where
    v * 255 + 0.5 crosses an integer (found by bisection on the restatement itself, in fp32)."""
    xs = []
    for k in range(lo + 1, hi + 1):
        a, b = np.float32(-3.0), np.float32(3.5)    # byte(a) < k <= byte(b): the rule is monotone in x

        def byte(x):
            img = np.zeros((3, 1, 1), np.float32)
            img[c] = x
            return int(image_tile(img)[0, 0, c])
        if not (byte(a) < k <= byte(b)):
            continue
        while True:
            nxt = np.nextafter(a, b, dtype=np.float32)
            if nxt >= b:
                break
            mid = np.float32((np.float64(a) + np.float64(b)) / 2)
            if mid <= a or mid >= b:
                mid = nxt
            if byte(mid) < k:
                a = mid
            else:
                b = mid
        xs += [np.nextafter(a, np.float32(-10), dtype=np.float32), a, b, np.nextafter(b, np.float32(10), dtype=np.float32)]
    return np.array(xs, np.float32)
