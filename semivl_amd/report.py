"""Evaluation report (cfg['eval_report']): the confusion matrix counted on the device, the metric table the mmseg papers
print beside mIoU, and the export of predictions as palette PNGs and of logits as files
(third_party/unimatch/eval.py:30-31,49-63: `--pred-path` / `--logit-path`).

`evaluate_report` is `evaluate` with ONE ops.confusion launch per batch into one device table [(K+1) x (K+1)]
(include/semivl_hip.h: svl_confusion_i64), a single all-reduce of that table when a process group is initialised and a single
copy to the host at the end; there is no per-image sync unless files are being written.  The table is a superset of
`svl_iou_hist_i64`'s three rows, so `EvalReport.miou` / `iou_class` are the floats `evaluate` returns.

The metric formulas are mmseg 0.x's `total_area_to_metrics`; mmseg is un-vendored, so this is a restatement (parity
unpinned).  With I = intersection, P = prediction area, T = target area per class:
    aAcc = sum I / sum T      IoU = I / (P + T - I)      Acc = Recall = I / T      Precision = I / P
    Dice = 2 I / (P + T)      Fscore = (1 + beta^2) Prec Rec / (beta^2 Prec + Rec)
means with nanmean, everything x 100 and unrounded; a zero denominator gives nan without a warning, `nan_to_num=v`
replaces nan afterwards.  Off unless asked for: nothing here is reached by `predict`, `evaluate` or a training step.
"""
import numbers
import os
import threading

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .evaluate import predict, tta_from_cfg

METRICS = ("mIoU", "mAcc", "mDice", "mFscore")
_FAMILY = {"mIoU": ("IoU",), "mAcc": ("Acc",), "mDice": ("Dice",), "mFscore": ("Fscore", "Precision", "Recall")}
_MODES = ("original", "center_crop", "padded_sliding_window", "zegclip_sliding_window", "sliding_window")


def eval_report_from_cfg(cfg):
    """cfg['eval_report'] -> None (key missing) or dict(metrics=tuple, beta=float, nan_to_num=None or float).  Keys, all
    optional: `metrics`: a list / tuple of names out of ('mIoU', 'mAcc', 'mDice', 'mFscore'), default ('mIoU',); `beta`: a
    real number > 0, default 1; `nan_to_num`: None or a real number.  Anything else raises a ValueError naming the offender."""
    if "eval_report" not in cfg:
        return None
    return _report_spec(cfg["eval_report"])


def _report_spec(spec):
    if not isinstance(spec, dict):
        raise ValueError(f"eval_report must be a dict, got {type(spec).__name__}")
    for k in spec:
        if k not in ("metrics", "beta", "nan_to_num"):
            raise ValueError(f"eval_report: unknown key {k!r}")
    metrics = spec.get("metrics", ("mIoU",))
    if isinstance(metrics, str) or not isinstance(metrics, (list, tuple)):
        raise ValueError(f"eval_report: metrics must be a list or tuple of names, got {metrics!r}")
    for m in metrics:
        if not isinstance(m, str) or m not in METRICS:
            raise ValueError(f"eval_report: unknown metric {m!r} (known: {', '.join(METRICS)})")
    beta = spec.get("beta", 1)
    if isinstance(beta, bool) or not isinstance(beta, numbers.Real) or not beta > 0:
        raise ValueError(f"eval_report: beta {beta!r} is not a real number > 0")
    ntn = spec.get("nan_to_num")
    if ntn is not None and (isinstance(ntn, bool) or not isinstance(ntn, numbers.Real)):
        raise ValueError(f"eval_report: nan_to_num {ntn!r} is neither None nor a real number")
    return dict(metrics=tuple(dict.fromkeys(metrics)), beta=float(beta), nan_to_num=None if ntn is None else float(ntn))


def voc_palette(n=256):
    """The PASCAL VOC colour map of n entries as a flat list [r0, g0, b0, r1, ...]: bit j of the class index's three
    interleaved bit streams becomes bit 7 - j of r, g and b."""
    out = []
    for i in range(n):
        r = g = b = 0
        c = i
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        out += [r, g, b]
    return out


def _check_palette(palette):
    if palette is None:
        return voc_palette(256)
    if isinstance(palette, (str, bytes)) or not hasattr(palette, "__len__") or not hasattr(palette, "__iter__"):
        raise ValueError(f"palette must be a flat sequence of ints, got {type(palette).__name__}")
    pal = list(palette)
    if len(pal) > 768 or len(pal) % 3 != 0:
        raise ValueError(f"palette: length {len(pal)} is not a multiple of 3 up to 768")
    for v in pal:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= 255:
            raise ValueError(f"palette: entry {v!r} is not an int in 0..255")
    return [int(v) for v in pal]


def _div(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


def _nanmean(x):
    ok = ~np.isnan(x)
    return float(x[ok].mean()) if ok.any() else float("nan")


class EvalReport:
    """The counts of one evaluation.  `table`: int64 [(K+1), (K+1)] (or flat), rows = annotation, columns = prediction, the
    last row / column for labels outside [0, K); `spec`: what `eval_report_from_cfg` returns (None: the defaults)."""

    def __init__(self, table, K, spec=None):
        K = int(K)
        tab = np.asarray(table)
        if tab.dtype != np.int64 or tab.size != (K + 1) ** 2:
            raise ValueError(f"EvalReport: table must hold {(K + 1) ** 2} int64 counts, got {tab.shape} {tab.dtype}")
        self.K = K
        self.table = tab.reshape(K + 1, K + 1).copy()
        self.spec = _report_spec({}) if spec is None else _report_spec(dict(spec))

    # -- counts
    @property
    def confusion(self):
        return self.table[:self.K, :self.K]

    @property
    def inter(self):
        return np.diagonal(self.table)[:self.K].copy()

    @property
    def pred_area(self):
        return self.table.sum(0)[:self.K]

    @property
    def target_area(self):
        return self.table.sum(1)[:self.K]

    # -- the reference's formula (x100, +1e-10): the floats `evaluate` returns
    @property
    def iou_class(self):
        h = np.concatenate([self.inter, self.pred_area, self.target_area]).astype(np.float64)
        K = self.K
        inter, union = h[:K], h[K:2 * K] + h[2 * K:] - h[:K]
        return inter / (union + 1e-10) * 100.0

    @property
    def miou(self):
        return float(np.mean(self.iou_class))

    # -- mmseg's metric table
    def metrics(self):
        """dict: 'aAcc' (float) and, per requested family, the per-class arrays [K] 'IoU' / 'Acc' / 'Dice' / 'Fscore',
        'Precision', 'Recall' with their nanmeans 'mIoU', 'mAcc', ...; x 100, unrounded."""
        I, P, T = (v.astype(np.float64) for v in (self.inter, self.pred_area, self.target_area))
        beta2 = self.spec["beta"] ** 2
        per = {}
        for m in self.spec["metrics"]:
            if m == "mIoU":
                per["IoU"] = _div(I, P + T - I) * 100.0
            elif m == "mAcc":
                per["Acc"] = _div(I, T) * 100.0
            elif m == "mDice":
                per["Dice"] = _div(2.0 * I, P + T) * 100.0
            else:
                prec, rec = _div(I, P), _div(I, T)
                per["Fscore"] = _div((1.0 + beta2) * prec * rec, beta2 * prec + rec) * 100.0
                per["Precision"], per["Recall"] = prec * 100.0, rec * 100.0
        out = {"aAcc": float(_div(I.sum(), T.sum()) * 100.0)}
        for k, v in per.items():
            out[k] = v
            out["m" + k] = _nanmean(v)
        ntn = self.spec["nan_to_num"]
        if ntn is not None:
            out = {k: (np.nan_to_num(v, nan=ntn) if isinstance(v, np.ndarray) else (ntn if np.isnan(v) else v))
                   for k, v in out.items()}
        return out

    def normalized(self, over="target"):
        """float64 [K, K] confusion divided by its row sums ('target'), column sums ('pred') or total ('all'); an empty row /
        column / matrix gives nan."""
        c = self.confusion.astype(np.float64)
        if over == "target":
            return _div(c, c.sum(1, keepdims=True))
        if over == "pred":
            return _div(c, c.sum(0, keepdims=True))
        if over == "all":
            return _div(c, c.sum())
        raise ValueError(f"normalized: over must be 'target', 'pred' or 'all', got {over!r}")

    def format_table(self, class_names=None):
        """The printable table: one line per class with the per-class metrics (2 decimals), then aAcc and the means."""
        if class_names is not None and len(class_names) != self.K:
            raise ValueError(f"format_table: {len(class_names)} class names for {self.K} classes")
        m = self.metrics()
        cols = [k for f in self.spec["metrics"] for k in _FAMILY[f]]
        names = [str(c) for c in (class_names if class_names is not None else range(self.K))]
        w = max([5] + [len(n) for n in names])
        lines = [" ".join(["Class".ljust(w)] + [c.rjust(9) for c in cols])]
        for k, n in enumerate(names):
            lines.append(" ".join([n.ljust(w)] + [f"{m[c][k]:.2f}".rjust(9) for c in cols]))
        lines.append(" ".join(["aAcc".ljust(w)] + ["m" + c for c in cols]))
        lines.append(" ".join([f"{m['aAcc']:.2f}".ljust(w)] + [f"{m['m' + c]:.2f}" for c in cols]))
        return "\n".join(lines)

    def to_dict(self):
        """A JSON-serialisable dict (plain ints, floats and lists; nan as None)."""
        def plain(v):
            if isinstance(v, np.ndarray):
                return [plain(x) for x in v.tolist()]
            if isinstance(v, list):
                return [plain(x) for x in v]
            if isinstance(v, float):
                return None if np.isnan(v) else v
            return v
        return dict(nclass=self.K, table=self.table.tolist(), miou=plain(self.miou), iou_class=plain(self.iou_class),
                    metrics={k: plain(v) for k, v in self.metrics().items()},
                    spec=dict(metrics=list(self.spec["metrics"]), beta=self.spec["beta"], nan_to_num=self.spec["nan_to_num"]))


class _FileWriter:
    """Export of predictions / logits: device -> pinned host copies with non_blocking=True and an event on the caller's
    stream; encoding and writing in `workers` host threads (PNG encoding releases the GIL); at most 2 x workers batches in
    flight; close() joins every writer and re-raises the first exception."""

    def __init__(self, pred_path, logit_path, palette, workers):
        from concurrent.futures import ThreadPoolExecutor
        self.pred_path, self.logit_path, self.palette = pred_path, logit_path, palette
        for p in (pred_path, logit_path):
            if p is not None:
                os.makedirs(p, exist_ok=True)
        workers = max(1, int(workers))
        self.pool = ThreadPoolExecutor(workers)
        self.slots = threading.BoundedSemaphore(2 * workers)
        self.futs = []

    def submit(self, pred, final, ids):
        ids = [ids] if ids is None or isinstance(ids, str) else list(ids)
        if len(ids) != pred.shape[0] or not all(isinstance(i, str) and len(i.split(" ")) == 2 for i in ids):
            raise ValueError(f"evaluate_report: writing files needs one id '<img> <lbl>' per sample, got {ids!r} for a batch "
                             f"of {pred.shape[0]}")
        names = [i.split(" ")[1].split("/")[-1] for i in ids]
        self.slots.acquire()
        try:
            host_pred = host_final = None
            if self.pred_path is not None:
                u8 = ops.label_u8(pred.contiguous())
                host_pred = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True).copy_(u8, non_blocking=True)
            if self.logit_path is not None:
                host_final = torch.empty(final.shape, dtype=final.dtype, pin_memory=True).copy_(final, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.futs.append(self.pool.submit(self._write, ev, host_pred, host_final, names))
        except BaseException:
            self.slots.release()
            raise

    def _write(self, ev, host_pred, host_final, names):
        try:
            ev.synchronize()
            for b, name in enumerate(names):
                if host_pred is not None:
                    from PIL import Image
                    arr = host_pred[b].numpy()
                    im = Image.new("P", (arr.shape[1], arr.shape[0]))
                    im.frombytes(arr.tobytes())
                    im.putpalette(self.palette)
                    im.save(os.path.join(self.pred_path, name))
                if host_final is not None:
                    torch.save(host_final[b:b + 1].clone(), os.path.join(self.logit_path, name).replace(".png", ".pt"))
        finally:
            self.slots.release()

    def close(self):
        self.pool.shutdown(wait=True)
        for f in self.futs:
            f.result()


def evaluate_report(model, loader, mode, cfg, tta=None, pred_path=None, logit_path=None, palette=None, workers=2):
    """`evaluate` with the whole confusion table: returns an EvalReport (spec from cfg['eval_report'], defaults when the key
    is missing).  `tta` as in `evaluate`.  `pred_path` / `logit_path` (eval.py:49-63): per sample, with id = '<img> <lbl>' as
    the loader yields it, the mode-'P' PNG os.path.join(pred_path, lbl.split('/')[-1]) of the ops.label_u8 indices with
    putpalette(palette), and torch.save of predict's `final` for that sample ([1, K, H, W], on the CPU, the same bits)
    under the same name with '.png' -> '.pt'.  `palette`: a flat sequence of at most 768 ints in 0..255, length divisible by
    3; None: voc_palette(256)."""
    spec = eval_report_from_cfg(cfg)
    if tta is None:
        tta = tta_from_cfg(cfg)
    if mode not in _MODES:
        raise ValueError(mode)
    K = cfg["nclass"]
    if pred_path is not None and K > 256:
        raise ValueError(f"evaluate_report: pred_path with nclass = {K} > 256: the class index does not fit a palette PNG")
    pal = _check_palette(palette)
    model.eval()
    writer = _FileWriter(pred_path, logit_path, pal, workers) if (pred_path is not None or logit_path is not None) else None
    table = None
    try:
        with torch.no_grad():
            for img, mask, ids in loader:
                img = img.cuda(non_blocking=True)
                mask = mask.cuda(non_blocking=True)
                if table is None:
                    table = ops.zeros(ops.confusion_len(K), dtype=torch.int64, device=img.device)
                pred, final = predict(model, img, mask, mode, cfg, return_logits=True, tta=tta)
                ops.confusion(pred.contiguous(), mask.contiguous(), K, 255, table)
                if writer is not None:
                    writer.submit(pred, final, ids)
    finally:
        if writer is not None:
            writer.close()
    if table is None:        # an empty shard still takes part in the all-reduce
        table = ops.zeros(ops.confusion_len(K), dtype=torch.int64)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(table)
    return EvalReport(table.cpu().numpy(), K, spec)
