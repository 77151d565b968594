"""svl_confusion_i64's table (include/semivl_hip.h), the three rows derived from it and the evaluation report's metrics
(semivl_amd/report.py: mmseg 0.x total_area_to_metrics, restated) with plain int64 / float64 torch and numpy ops, on
whatever device the inputs live on.  The reference of tests/test_confusion_kernels_gpu.py and tests/test_evalreport_*.py;
itself held to the reference project's own intersectionAndUnion by tests/test_evalreport_ref.py."""
import numpy as np
import torch


def table_len(K):
    return (K + 1) * (K + 1)


def confusion_ref(pred, target, K, ignore_index=255):
    """The table int64 [(K+1)^2] of ONE call on a zeroed table: bincount of the pair key after the clamp."""
    p, t = pred.reshape(-1), target.reshape(-1)
    keep = t != ignore_index
    r = torch.where((t >= 0) & (t < K), t, torch.full_like(t, K))
    c = torch.where((p >= 0) & (p < K), p, torch.full_like(p, K))
    key = (r * (K + 1) + c)[keep]
    return torch.bincount(key, minlength=table_len(K))[:table_len(K)].to(torch.int64)


def derived_rows(table, K):
    """(intersection, prediction area, target area), int64 [K] each, of a table [(K+1)^2] (torch or numpy)."""
    tab = table.reshape(K + 1, K + 1)
    inter = tab.diagonal()[:K] if isinstance(tab, torch.Tensor) else np.diagonal(tab)[:K]
    return inter, tab.sum(0)[:K], tab.sum(1)[:K]


def _div(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


def _nanmean(x):
    ok = ~np.isnan(x)
    return float(x[ok].mean()) if ok.any() else float("nan")


def metrics_ref(inter, pred_area, target_area, metrics=("mIoU",), beta=1, nan_to_num=None):
    """The report's metric dict from the three rows: per-class arrays x 100 (nan on a zero denominator), their nanmeans
    under the 'm' names, and aAcc."""
    I, P, T = (np.asarray(v, np.float64) for v in (inter, pred_area, target_area))
    out = {"aAcc": _div(I.sum(), T.sum()) * 100.0}
    for m in metrics:
        if m == "mIoU":
            out["IoU"] = _div(I, P + T - I) * 100.0
        elif m == "mAcc":
            out["Acc"] = _div(I, T) * 100.0
        elif m == "mDice":
            out["Dice"] = _div(2 * I, P + T) * 100.0
        elif m == "mFscore":
            prec, rec = _div(I, P), _div(I, T)
            out["Fscore"] = _div((1 + beta ** 2) * prec * rec, beta ** 2 * prec + rec) * 100.0
            out["Precision"], out["Recall"] = prec * 100.0, rec * 100.0
        else:
            raise ValueError(m)
    for k in [k for k in out if k != "aAcc"]:
        out["m" + k] = _nanmean(out[k])
    out["aAcc"] = float(out["aAcc"])
    if nan_to_num is not None:
        out = {k: (np.nan_to_num(v, nan=nan_to_num) if isinstance(v, np.ndarray) else (nan_to_num if np.isnan(v) else v))
               for k, v in out.items()}
    return out


def label_maps(n, K, seed, run=0):
    """(pred, target) int64 [n] on the CPU: annotations of K classes (runs of `run` pixels of one class when run > 0), a
    prediction that is right on about 60 % of them, and a sprinkle of 255 / 254 / -1 targets and -1 / 255 / K predictions."""
    g = torch.Generator().manual_seed(seed)
    if run:
        t = torch.randint(0, K, ((n + run - 1) // run,), generator=g).repeat_interleave(run)[:n].clone()
    else:
        t = torch.randint(0, K, (n,), generator=g)
    p = torch.where(torch.rand(n, generator=g) < 0.6, t, torch.randint(0, K, (n,), generator=g))
    u = torch.rand(n, generator=g)
    t = torch.where(u < 0.08, torch.full_like(t, 255), t)
    t = torch.where((u >= 0.08) & (u < 0.10), torch.full_like(t, 254), t)
    t = torch.where((u >= 0.10) & (u < 0.11), torch.full_like(t, -1), t)
    v = torch.rand(n, generator=g)
    p = torch.where(v < 0.01, torch.full_like(p, -1), p)
    p = torch.where((v >= 0.01) & (v < 0.02), torch.full_like(p, 255), p)
    p = torch.where((v >= 0.02) & (v < 0.03), torch.full_like(p, K), p)
    return p, t
