"""Evaluation path: sliding-window inference + mIoU, mirroring
third_party/unimatch/supervised.py:40-164 (`predict`, `evaluate`) and util/utils.py:91-103 (`intersectionAndUnion`).

Same `predict(model, img, mask, mode, cfg)` signature and modes.  Window logits are accumulated on the GPU with the
library's strided copy kernel, the confusion counts are integer histograms on the device, and the per-image
3 x all_reduce of the reference is replaced by ONE all_reduce of the summed int64 counts (integer sums commute, so the
result is identical).  Optional multi-scale + flip test-time augmentation (`tta`, cfg['eval_tta']): see `predict`.
"""
import numbers

import numpy as np
import torch
import torch.distributed as dist

from . import ops


def _crop(img, y1, y2, x1, x2):
    """img[:, :, y1:y2, x1:x2] as a contiguous tensor (strided row copy)."""
    b, c, h, w = img.shape
    ch, cw = y2 - y1, x2 - x1
    out = ops.empty(b, c, ch, cw, device=img.device)
    ops.copy2d(img, y1 * w + x1, ch, h * w, w, out, 0, ch, ch * cw, cw, b * c * ch, cw)
    return out


def _window_add(canvas, win, y1, x1):
    """canvas[:, :, y1:y1+ch, x1:x1+cw] += win."""
    b, n, h, w = canvas.shape
    ch, cw = win.shape[2:]
    ops.copy2d(win.contiguous(), 0, ch, ch * cw, cw, canvas, y1 * w + x1, ch, h * w, w, b * n * ch, cw, accumulate=True)


def _view_scores(model, img, mask_hw, mode, cfg):
    """The single-view body of `predict`: the `final` class map of one view of the image (logits for 'original', 'center_crop'
    and 'zegclip_sliding_window', summed window probabilities for the two other sliding-window modes)."""
    img = img.contiguous()
    if mode == "zegclip_sliding_window":  # supervised.py:70-102
        hs = ws = cfg["stride"]
        hc = wc = cfg["crop_size"]
        b, _, h, w = img.shape
        K = cfg["nclass"]
        hg = max(h - hc + hs - 1, 0) // hs + 1
        wg = max(w - wc + ws - 1, 0) // ws + 1
        preds = ops.zeros(b, K, h, w, device=img.device)
        count = ops.zeros(b, 1, h, w, device=img.device)
        for hi in range(hg):
            for wi in range(wg):
                y1, x1 = hi * hs, wi * ws
                y2, x2 = min(y1 + hc, h), min(x1 + wc, w)
                y1, x1 = max(y2 - hc, 0), max(x2 - wc, 0)
                logit = model(_crop(img, y1, y2, x1, x2))
                _window_add(preds, logit, y1, x1)
                ones = ops.fill(ops.empty(b, 1, y2 - y1, x2 - x1, device=img.device), 1.0)
                _window_add(count, ones, y1, x1)
        cnt = count.expand(b, K, h, w).contiguous() if K > 1 else count
        preds = ops.eltwise(7, preds.view(-1), cnt.view(-1)).view(b, K, h, w)
        H, W = mask_hw
        final = ops.bilinear_planes_fwd(preds, h, w, True, H, W) if (H, W) != (h, w) else preds
    elif mode == "sliding_window":  # supervised.py:104-117: softmax-probability accumulation, stride int(2/3 crop)
        grid = cfg["crop_size"]
        b, _, h, w = img.shape
        final = ops.zeros(b, cfg["nclass"], h, w, device=img.device)
        step = int(grid * 2 / 3)
        row = 0
        while row < h:
            col = 0
            while col < w:
                y2, x2 = min(h, row + grid), min(w, col + grid)
                logit = model(_crop(img, row, y2, col, x2))
                _window_add(final, ops.softmax_planes(logit.contiguous()), row, col)
                col += step
            row += step
    elif mode == "padded_sliding_window":  # supervised.py:41-68: zero-padded crops, configurable stride
        grid, stride = cfg["crop_size"], cfg["stride"]
        if stride < 1:
            stride = int(grid * stride)
        b, c, h, w = img.shape
        final = ops.zeros(b, cfg["nclass"], h, w, device=img.device)
        row = 0
        while row < h:
            col = 0
            while col < w:
                y2, x2 = min(h, row + grid), min(w, col + grid)
                ch, cw = y2 - row, x2 - col
                padded = ops.zeros(b, c, grid, grid, device=img.device)
                ops.copy2d(img, row * w + col, ch, h * w, w, padded, 0, ch, grid * grid, grid, b * c * ch, cw)
                prob = ops.softmax_planes(model(padded).contiguous())
                _window_add(final, _crop(prob, 0, ch, 0, cw), row, col)
                col += stride
            row += stride
    elif mode in ("original", "center_crop"):
        if mode == "center_crop":
            h, w = img.shape[-2:]
            sh, sw = (h - cfg["crop_size"]) // 2, (w - cfg["crop_size"]) // 2
            img = _crop(img, sh, sh + cfg["crop_size"], sw, sw + cfg["crop_size"])
        final = model(img)
    else:
        raise ValueError(mode)
    return final


_TTA_KIND = {"original": 0, "zegclip_sliding_window": 0, "sliding_window": 1, "padded_sliding_window": 1}


def tta_from_cfg(cfg):
    """cfg['eval_tta'] -> None or dict(ratios=tuple, flip=bool).  Keys: `ratios` (or mmseg's spelling `img_ratios`, not both):
    a non-empty list / tuple of real numbers > 0, default (1.0,); `flip`: bool, default False; `flip_direction`: only
    'horizontal'.  Anything else raises."""
    return _tta_spec(cfg.get("eval_tta"))


def _tta_spec(tta):
    if tta is None:
        return None
    if not isinstance(tta, dict):
        raise ValueError(f"eval_tta must be a dict or None, got {type(tta).__name__}")
    for k in tta:
        if k not in ("ratios", "img_ratios", "flip", "flip_direction"):
            raise ValueError(f"eval_tta: unknown key {k!r}")
    if "ratios" in tta and "img_ratios" in tta:
        raise ValueError("eval_tta: give 'ratios' or 'img_ratios', not both")
    if tta.get("flip_direction", "horizontal") != "horizontal":
        raise NotImplementedError(f"eval_tta: flip_direction {tta['flip_direction']!r} (only 'horizontal')")
    ratios = tta.get("ratios", tta.get("img_ratios", (1.0,)))
    if not isinstance(ratios, (list, tuple)) or len(ratios) == 0:
        raise ValueError(f"eval_tta: ratios must be a non-empty list or tuple, got {ratios!r}")
    for r in ratios:
        if isinstance(r, bool) or not isinstance(r, numbers.Real) or not r > 0:
            raise ValueError(f"eval_tta: ratio {r!r} is not a real number > 0")
    flip = tta.get("flip", False)
    if not isinstance(flip, bool):
        raise ValueError(f"eval_tta: flip must be a bool, got {flip!r}")
    return dict(ratios=tuple(float(r) for r in ratios), flip=flip)


def predict(model, img, mask, mode, cfg, return_logits=False, tta=None):
    """supervised.py:40-133.  `tta` (a dict as `tta_from_cfg` accepts, or None): multi-scale + flip test-time augmentation
    with the semantics of mmseg 0.x MultiScaleFlipAug + EncoderDecoder.aug_test.  For each ratio in the given order,
    unflipped then (with flip) mirrored, the single-view body runs on ops.tta_view(img, int(h r + 0.5), int(w r + 0.5), flip)
    (mmcv.rescale_size's rounding; the image is already the normalised float tensor here, so the resize is ATen's bilinear
    with align_corners = False, not OpenCV's on the uint8 image), its `final` is resized to mask.shape[-2:] with the model's
    align_corners, turned into class scores (softmax of logits; probability sums over their total), un-flipped and averaged
    over the n views in one pass per view (ops.tta_accum).  Returns the argmax of the mean scores, and with return_logits
    the mean scores [B, K, H, W] themselves."""
    tta = _tta_spec(tta)
    if tta is None:
        final = _view_scores(model, img, mask.shape[-2:], mode, cfg)
    else:
        if mode not in _TTA_KIND:
            if mode == "center_crop":
                raise ValueError("center_crop with tta: the views would cover different regions")
            raise ValueError(mode)
        img = img.contiguous()
        h, w = img.shape[-2:]
        H, W = mask.shape[-2:]
        align = getattr(model, "align_corners", False)
        views = [(r, f) for r in tta["ratios"] for f in ((False, True) if tta["flip"] else (False,))]
        final = ops.empty(img.shape[0], cfg["nclass"], H, W, device=img.device)
        for i, (r, f) in enumerate(views):
            view = ops.tta_view(img, int(h * r + 0.5), int(w * r + 0.5), f)
            scores = _view_scores(model, view, (H, W), mode, cfg)
            ops.tta_accum(scores.contiguous(), final, _TTA_KIND[mode], align, f, 1.0 / len(views), i > 0)
    _, pred = ops.softmax_max(final.contiguous())  # argmax over classes (first max wins, like torch.argmax)
    return (pred, final) if return_logits else pred


def intersection_and_union(pred, target, K, ignore_index=255, hist=None):
    """Device version of intersectionAndUnion: returns (area_intersection, area_union, area_target) int64 [K]."""
    own = hist is None
    if own:
        hist = ops.zeros(3 * K, dtype=torch.int64, device=pred.device)
    ops.iou_hist(pred.contiguous(), target.contiguous(), K, ignore_index, hist)
    if not own:
        return None
    inter, out, tgt = hist[:K], hist[K:2 * K], hist[2 * K:]
    return inter, out + tgt - inter, tgt


def evaluate(model, loader, mode, cfg, tta=None):
    """supervised.py:135-164.  Returns (mIoU, iou_class) with the reference's formula (x100, +1e-10).  `tta`: test-time
    augmentation as in `predict`; defaults to cfg['eval_tta'] (`tta_from_cfg`)."""
    if tta is None:
        tta = tta_from_cfg(cfg)
    model.eval()
    assert mode in ["original", "center_crop", "padded_sliding_window", "zegclip_sliding_window", "sliding_window"]
    K = cfg["nclass"]
    hist = None
    with torch.no_grad():
        for img, mask, _ in loader:
            img = img.cuda(non_blocking=True)
            mask = mask.cuda(non_blocking=True)
            if hist is None:
                hist = ops.zeros(3 * K, dtype=torch.int64, device=img.device)
            pred = predict(model, img, mask, mode, cfg, tta=tta)
            intersection_and_union(pred, mask, K, 255, hist)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(hist)
    h = hist.cpu().numpy().astype(np.float64)
    inter, union = h[:K], h[K:2 * K] + h[2 * K:] - h[:K]
    iou_class = inter / (union + 1e-10) * 100.0
    return float(np.mean(iou_class)), iou_class
