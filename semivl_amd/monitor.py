"""Pseudo-label and guidance quality meter of the semi-supervised step, counted on the device.

What one watches first in a UniMatch / SemiVL run: the share of unlabelled pixels above `conf_thresh` (UniMatch's
`mask_ratio`, semivl.py:280-281), how often the MaskCLIP guidance speaks and agrees with the pseudo-label, and -- on the
benchmarks, where the "unlabelled" images do have annotations (the reference's `pleval`, semivl.py:115) -- the mIoU of the
pseudo-labels, of the confident pseudo-labels and of the guidance against the held-back ground truth.

`semivl_train_step(..., monitor=meter)` hands the label maps the step trains on to `PseudoLabelMeter.update` (ONE
svl_pl_stats_i64 launch on the step's stream) and its loss vector to `add_losses` (one more); nothing is read back until
`report()`, the only sync.  Table layout: include/semivl_hip.h at svl_pl_stats_i64.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import ops

ROWS = ("pl_area", "plc_area", "mc_area", "agree", "gt_area", "pl_inter", "pl_area_gt", "plc_gt_area", "plc_inter",
        "plc_area_gt", "mc_gt_area", "mc_inter", "mc_area_gt")
_KEYS = ("conf_bins", "gt")


def pl_monitor_from_cfg(cfg):
    """cfg['pl_monitor'] = dict(conf_bins=20, gt=True) -> dict(conf_bins, gt) with the defaults filled in (conf_bins 20,
    gt False), or None when the key is missing.  conf_bins: an int >= 1 (no bool); gt: a bool -- also hand the unlabelled
    images' annotations through the loader (GpuAugmenter.unlabeled_gt) and count against them."""
    if "pl_monitor" not in cfg:
        return None
    spec = cfg["pl_monitor"]
    if not isinstance(spec, dict):
        raise ValueError(f"pl_monitor: expected a dict with the keys {_KEYS}, got {spec!r}")
    for k in spec:
        if k not in _KEYS:
            raise ValueError(f"pl_monitor: unknown key {k!r} (known: {_KEYS})")
    bins = spec.get("conf_bins", 20)
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 1:
        raise ValueError(f"pl_monitor: conf_bins must be an int >= 1, got {bins!r}")
    gt = spec.get("gt", False)
    if not isinstance(gt, bool):
        raise ValueError(f"pl_monitor: gt must be a bool, got {gt!r}")
    return dict(conf_bins=int(bins), gt=gt)


def _div(a, b):
    """a / b in float64, nan where b == 0, no warning."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


def _iou(inter, area, target):
    """intersection / (area + target - intersection) per class, and its mean over the classes with a non-zero union."""
    union = area + target - inter
    iou = _div(inter, union)
    seen = union != 0
    return iou, (float(iou[seen].mean()) if seen.any() else float("nan"))


def report_from_table(table, num_classes, bins, loss_sum=None, steps=0):
    """The derived values of `PseudoLabelMeter.report` from a host copy of the table (int64 [13 N + 2 bins + 1])."""
    from .train import LOSS_NAMES
    N = int(num_classes)
    table = np.asarray(table, np.int64).reshape(-1)
    assert table.size == ops.pl_stats_len(N, bins), (table.size, N, bins)
    r = {name: table[i * N:(i + 1) * N] for i, name in enumerate(ROWS)}
    hist = table[13 * N:13 * N + bins]
    hist_ok = table[13 * N + bins:13 * N + 2 * bins]
    valid, mc_n = int(r["pl_area"].sum()), int(r["mc_area"].sum())
    out = dict(steps=int(steps), pixels=int(table[-1]),
               mask_ratio=float(_div(r["plc_area"].sum(), valid)),
               guidance_coverage=float(_div(mc_n, valid)),
               guidance_agreement=float(_div(r["agree"].sum(), mc_n)),
               pl_class_freq=_div(r["pl_area"], valid), guidance_class_freq=_div(r["mc_area"], mc_n),
               conf_hist=hist.copy(), table=table.copy())
    if loss_sum is not None:
        means = _div(np.asarray(loss_sum, np.float64), float(steps))
        for i, name in enumerate(LOSS_NAMES):
            out["train/" + name] = float(means[i])
    if int(r["gt_area"].sum()) > 0:
        out["pl_iou"], out["pl_miou"] = _iou(r["pl_inter"], r["pl_area_gt"], r["gt_area"])
        out["confident_pl_iou"], out["confident_pl_miou"] = _iou(r["plc_inter"], r["plc_area_gt"], r["plc_gt_area"])
        out["guidance_iou"], out["guidance_miou"] = _iou(r["mc_inter"], r["mc_area_gt"], r["mc_gt_area"])
        out["pl_acc_per_bin"] = _div(hist_ok, hist)
    return out


class PseudoLabelMeter:
    """The table (int64), the sum of the steps' loss vectors (float64 [8]) and the step count, all on `device`."""

    def __init__(self, num_classes, conf_bins=20, device="cuda"):
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or num_classes < 1:
            raise ValueError(f"PseudoLabelMeter: num_classes must be an int >= 1, got {num_classes!r}")
        if isinstance(conf_bins, bool) or not isinstance(conf_bins, (int, np.integer)) or conf_bins < 1:
            raise ValueError(f"PseudoLabelMeter: conf_bins must be an int >= 1, got {conf_bins!r}")
        self.num_classes, self.conf_bins, self.device = int(num_classes), int(conf_bins), torch.device(device)
        n = ops.pl_stats_len(self.num_classes, self.conf_bins)
        self._counts = ops.zeros(n + 1, dtype=torch.int64, device=self.device)       # the table, then the step counter
        self.table, self.steps = self._counts[:n], self._counts[n:]
        self.loss_sum = ops.zeros(8, dtype=torch.float64, device=self.device)
        self.conf_thresh = None

    @classmethod
    def from_cfg(cls, cfg, num_classes, device="cuda"):
        """A meter for cfg['pl_monitor'], or None when the key is missing."""
        spec = pl_monitor_from_cfg(cfg)
        return None if spec is None else cls(num_classes, spec["conf_bins"], device)

    def update(self, mask_w, conf_w, ignore_mask, conf_thresh, mclip=None, mask_u=None):
        """Count one batch: pseudo-labels, their confidence, the padding mask, optionally the guidance and the held-back
        annotation (int64 [B, H, W], conf fp32).  One launch on the current stream, no sync."""
        thresh = float(conf_thresh)
        if self.conf_thresh is not None and thresh != self.conf_thresh:
            raise ValueError(f"PseudoLabelMeter.update: conf_thresh changed from {self.conf_thresh!r} to {thresh!r}; the rows "
                             f"of confident pixels would mix two thresholds -- reset() first")
        shape = tuple(mask_w.shape)
        for name, t_, dt in (("mask_w", mask_w, torch.int64), ("conf_w", conf_w, torch.float32),
                             ("ignore_mask", ignore_mask, torch.int64), ("mclip", mclip, torch.int64),
                             ("mask_u", mask_u, torch.int64)):
            if t_ is not None and (t_.dtype != dt or tuple(t_.shape) != shape):
                raise ValueError(f"PseudoLabelMeter.update: {name} is {tuple(t_.shape)} {t_.dtype}, expected {shape} {dt}")
        c = lambda t_: None if t_ is None else t_.contiguous()
        ops.pl_stats(c(mask_w), c(conf_w), c(ignore_mask), self.table, self.num_classes, self.conf_bins, thresh,
                     mc=c(mclip), gt=c(mask_u))
        self.conf_thresh = thresh

    def add_losses(self, losses):
        """Add the step's loss vector (device fp32 [8], LOSS_NAMES order) into the sum and count the step.  No sync."""
        if losses.dtype != torch.float32 or losses.numel() != 8:
            raise ValueError(f"PseudoLabelMeter.add_losses: expected fp32 [8], got {tuple(losses.shape)} {losses.dtype}")
        ops.pl_add_losses(losses.contiguous(), self.loss_sum, self.steps)

    def report(self, reduce=True):
        """The only sync: the counts summed over the ranks of an initialised process group (`reduce`; the meter's own
        state stays per-rank), one copy to the host, the derived values as plain Python / numpy values, `table` included."""
        counts, loss_sum = self._counts, self.loss_sum
        if reduce and dist.is_available() and dist.is_initialized():
            counts, loss_sum = counts.clone(), loss_sum.clone()
            dist.all_reduce(counts)
            dist.all_reduce(loss_sum)
        host = counts.cpu().numpy()
        return report_from_table(host[:-1], self.num_classes, self.conf_bins, loss_sum.cpu().numpy(), int(host[-1]))

    def reset(self):
        """Zero everything on the device; the next update may use another conf_thresh."""
        for t_ in (self._counts, self.loss_sum):
            if t_.is_cuda:
                ops.fill(t_.view(torch.float32), 0.0)
            else:
                t_.zero_()
        self.conf_thresh = None
