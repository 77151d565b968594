"""Debug panels of a training run, rendered on the device (semivl.py:371-406, utils/plot_utils.py).

The reference pulls twelve to sixteen full-resolution tensors per sample to the host once per epoch and draws them with
matplotlib.  Here `semivl_train_step(..., panel=StepPanel(...))` hands the same tensors to two kernels
(include/semivl_hip.h: svl_panel_image_u8, svl_panel_label_u8) that fill ONE u8 canvas [B, rows * H, 4 * W, 3] on the
step's stream; the canvas crosses to pinned host memory with one asynchronous copy and writer threads encode one PNG per
sample.  The step thread never waits for the files; `close()` joins the writers and re-raises their first error.

Layout (the reference's order; rows = 3, or 4 with the MaskCLIP guidance):

    Image L    Image S1   Image S2   Image FP        the four images after CutMix, de-normalised
    Pred L     Pred S1    Pred S2    Pred FP         argmax of the logits (the step's own softmax-max kernel)
    GT L       PL S1      PL S2      PL FP           mask_x, the two mixed pseudo-label maps, mask_w
    (white)    MC S1      MC S2      MC FP           the two mixed guidance maps, mclip

Labels outside the palette (254, 255, negative, >= K) are white, as plot_utils.py's colorize_label leaves them.  The
palette is cfg['palette'] (a flat list, report._check_palette's rules) or report.voc_palette(256).
"""
import os
import threading

import torch

from . import ops
from .data import MEAN, STD
from .report import _check_palette

COLS = 4


def palette_from_cfg(cfg):
    """cfg['palette'] (optional: a flat sequence [r0, g0, b0, r1, ...] of at most 256 colours) -> the validated flat list;
    report.voc_palette(256) without the key."""
    pal = _check_palette(cfg.get("palette"))
    if len(pal) == 0:
        raise ValueError("palette: needs at least one colour")
    return pal


def canvas_shape(B, H, W, guided):
    return (B, (4 if guided else 3) * H, COLS * W, 3)


class StepPanel:
    """StepPanel(out_dir, palette=None, rank=0, workers=2, mean=data.MEAN, std=data.STD).  One instance serves a whole
    run: every `capture` renders one canvas and queues its files `out_dir/{iters:07d}_{rank}-{b}.png`.  After a capture
    `canvas` is the device canvas (uint8 [B, rows * H, 4 * W, 3]) and `files` the paths being written."""

    def __init__(self, out_dir, palette=None, rank=0, workers=2, mean=MEAN, std=STD):
        from concurrent.futures import ThreadPoolExecutor
        self.out_dir, self.rank = str(out_dir), int(rank)
        self.palette = _check_palette(palette)
        if len(self.palette) == 0:
            raise ValueError("palette: needs at least one colour")
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError(f"StepPanel: mean and std must hold 3 numbers each, got {mean!r} and {std!r}")
        workers = max(1, int(workers))
        self.pool = ThreadPoolExecutor(workers)
        self.slots = threading.BoundedSemaphore(2 * workers)
        self.futs, self.canvas, self.files = [], None, []
        self._dev = {}      # device -> (palette u8 [K, 3], the one-colour white palette)

    def _palettes(self, dev):
        if dev not in self._dev:
            pal = torch.tensor(self.palette, dtype=torch.uint8).view(-1, 3)
            self._dev[dev] = (pal.to(dev), torch.full((1, 3), 255, dtype=torch.uint8).to(dev))
        return self._dev[dev]

    def render(self, images, label_rows):
        """The canvas of `images` (4 fp32 [B, 3, H, W]) and `label_rows` (2 or 3 rows of 4 int64 [B, H, W]; None = a white
        tile): 4 + 4 * len(label_rows) launches on the current stream, no sync."""
        if len(images) != COLS or any(len(r) != COLS for r in label_rows) or len(label_rows) not in (2, 3):
            raise ValueError(f"StepPanel: expected 4 images and 2 or 3 rows of 4 label maps, got {len(images)} images and rows "
                             f"of {[len(r) for r in label_rows]}")
        B, _, H, W = images[0].shape
        dev = images[0].device
        pal, white = self._palettes(dev)
        canvas = torch.empty(canvas_shape(B, H, W, len(label_rows) == 3), dtype=torch.uint8, device=dev)
        for j, img in enumerate(images):
            ops.panel_image(img.contiguous(), self.mean, self.std, canvas, 0, j * W)
        some_map = next(m for r in label_rows for m in r if m is not None)
        for i, row in enumerate(label_rows):
            for j, m in enumerate(row):
                if m is None:       # every label is outside a one-colour palette's range or is that colour: white
                    ops.panel_label(some_map.contiguous(), white, canvas, (1 + i) * H, j * W)
                else:
                    ops.panel_label(m.contiguous(), pal, canvas, (1 + i) * H, j * W)
        return canvas

    def capture(self, iters, images, label_rows):
        """Render, start the copy to pinned host memory and queue the PNG files of step `iters`; returns the device canvas."""
        canvas = self.render(images, label_rows)
        os.makedirs(self.out_dir, exist_ok=True)
        files = [os.path.join(self.out_dir, f"{int(iters):07d}_{self.rank}-{b}.png") for b in range(canvas.shape[0])]
        self.slots.acquire()
        try:
            host = torch.empty(canvas.shape, dtype=torch.uint8, pin_memory=True).copy_(canvas, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.futs.append(self.pool.submit(self._write, ev, host, files))
        except BaseException:
            self.slots.release()
            raise
        self.canvas, self.files = canvas, files
        return canvas

    def _write(self, ev, host, files):
        try:
            from PIL import Image
            ev.synchronize()
            for b, path in enumerate(files):
                Image.fromarray(host[b].numpy(), "RGB").save(path)
        finally:
            self.slots.release()

    def close(self):
        """Join the writers; the first exception one of them raised is raised here."""
        self.pool.shutdown(wait=True)
        futs, self.futs = self.futs, []
        for f in futs:
            f.result()
