"""The SemiVL training steps on MI355X: the reference-named loss helpers, the step's streams, what both steps share (CELoss
setup, stream override, head resolution, the head's memory plan, CE dispatch, the backward + update tail), the labelled-only
step, the semi-supervised step as a sequence of phases and the gradient all-reduce; the optimizers are re-exported from optim.py.

Mirrors (same names / argument meaning):
  utils/train_utils.py:19-49   cutmix_img_, cutmix_mask, confidence_weighted_loss
  semivl.py:52-58              compute_mc_loss
  semivl.py:223-345            the loop body  -> semivl_train_step()
  supervised.py:268-301        the labelled-only loop body -> supervised_train_step()
  semivl.py:118-125,330-345    the optimizers + poly LR -> optim.py (FusedAdamW, FusedSGD)
  semivl.py:139-140            DistributedDataParallel -> GradAllReducer (RCCL all-reduce of the flat grad arena)
"""

import contextlib
import numbers
import os
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .optim import (FusedAdamW, FusedSGD, build_optimizer, ema_from_cfg, grad_clip_from_cfg,  # noqa: F401
                    mmcv_param_groups, optimizer_from_cfg, sgd_original_groups, sgd_original_lr)


# ------------------------------------------------------------------------------------------------ reference-named helpers
def cutmix_img_(img, img_mix, cutmix_box):
    """In place: img[box == 1] = img_mix[box == 1] (train_utils.py:19-21), one select kernel, no host sync."""
    ops.cutmix_f32(img, img_mix, cutmix_box, out=img)


def cutmix_mask(mask, mask_mix, cutmix_box):
    """train_utils.py:24-27 for int64 label-like maps and fp32 confidence maps."""
    if mask.dtype == torch.int64:
        return ops.cutmix_i64(mask, mask_mix, cutmix_box)
    return ops.cutmix_f32(mask, mask_mix, cutmix_box)


def confidence_weighted_loss(loss, conf_map, ignore_mask, cfg):
    """train_utils.py:30-49 on an autograd-tracked per-pixel loss map.  API-compatibility helper for callers that
    compute the per-pixel CE themselves; `semivl_train_step` uses the fused CE kernel instead."""
    assert loss.dim() == 3 and conf_map.dim() == 3 and ignore_mask.dim() == 3
    valid_mask = ignore_mask != 255
    sum_pixels = dict(dim=(1, 2), keepdim=True)
    if cfg["conf_mode"] == "pixelwise":
        loss = loss * ((conf_map >= cfg["conf_thresh"]) & valid_mask)
        return loss.sum() / valid_mask.sum().item()
    if cfg["conf_mode"] == "pixelratio":
        r = ((conf_map >= cfg["conf_thresh"]) & valid_mask).sum(**sum_pixels) / valid_mask.sum(**sum_pixels)
        return (loss * r).sum() / valid_mask.sum().item()
    if cfg["conf_mode"] == "pixelavg":
        avg_conf = (conf_map * valid_mask).sum(**sum_pixels) / valid_mask.sum(**sum_pixels)
        return (loss.sum() * avg_conf).sum() / valid_mask.sum().item()
    raise ValueError(cfg["conf_mode"])


def compute_mc_loss(pred, mask, ign, mcc_loss_reduce="mean_all", criterion_mc=None):
    """semivl.py:52-58 (MaskCLIP guidance loss).  The reference reads `criterion_mc` / `mcc_loss_reduce` from module
    globals set in main() (semivl.py:158-164); here they are arguments with the same meaning: reduce 'mean' ->
    nn.CrossEntropyLoss(ignore_index=255), 'mean_valid' / 'mean_all' -> the per-pixel map (reduction='none') summed and
    divided by the number of non-ignored pixels / by all pixels.  API-compatibility helper: an autograd-tracked scalar for
    callers that write the loop body themselves; `semivl_train_step` uses the fused CE kernel instead."""
    if criterion_mc is None:
        criterion_mc = (torch.nn.CrossEntropyLoss(ignore_index=255) if mcc_loss_reduce == "mean" else
                        torch.nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    l_mc = criterion_mc(pred, mask)
    if mcc_loss_reduce == "mean_valid":
        l_mc = l_mc.sum() / (ign != 255).sum()
    elif mcc_loss_reduce == "mean_all":
        l_mc = l_mc.sum() / ign.numel()
    elif mcc_loss_reduce != "mean":
        raise ValueError(mcc_loss_reduce)
    return l_mc


class ProbOhemCrossEntropy2d(torch.nn.Module):
    """third_party/unimatch/util/ohem.py's criterion (the reference's cfg['criterion'] = 'OHEM', semivl.py:142-149) with
    its constructor signature.  API-compatibility helper for reference-style scripts: the hard pixels are selected on the
    device by the OHEM kernels (ops.ohem_target, no host sync), then the mean cross entropy over the kept pixels is taken
    like the reference's inner nn.CrossEntropyLoss(ignore_index).  `semivl_train_step` reads the same configuration and
    relabels through the same kernels before its fused cross entropy.
    Supported: ignore_index 255 (the CE kernels fix it), reduction 'mean', use_weight False; `down_ratio` is accepted and
    unused, as in the reference."""

    def __init__(self, ignore_index, reduction="mean", thresh=0.7, min_kept=256, down_ratio=1, use_weight=False):
        super().__init__()
        if ignore_index != 255:
            raise ValueError(f"ProbOhemCrossEntropy2d: ignore_index={ignore_index!r}; the cross-entropy kernels fix it at 255")
        if reduction != "mean":
            raise NotImplementedError(f"ProbOhemCrossEntropy2d: reduction={reduction!r}; only 'mean' is supported")
        if use_weight:
            raise NotImplementedError("ProbOhemCrossEntropy2d: use_weight=True (the 19 fixed class weights) is not supported")
        self.ignore_index = ignore_index
        self.thresh = float(thresh)
        self.min_kept = int(min_kept)
        self.down_ratio = down_ratio

    def relabel(self, pred, target, up=None, counts_out=None):
        """The relabelled int64 target (255 outside the kept pixels); `up` as in ops.ohem_target."""
        return ops.ohem_target(pred.detach(), target, self.thresh, self.min_kept, up=up, counts_out=counts_out)

    def forward(self, pred, target):
        return torch.nn.functional.cross_entropy(pred, self.relabel(pred, target), ignore_index=self.ignore_index)


def supervised_criterion(cfg):
    """cfg['criterion'] (semivl.py:142-149) -> None for the plain cross entropy (missing, 'CELoss', and -- unchanged --
    every other name) or a ProbOhemCrossEntropy2d for 'OHEM', built from cfg['criterion']['kwargs'] as given (ohem.py's
    defaults fill the rest, like the reference).  The `label_smoothing` / `weight` kwargs of 'CELoss' are read by
    celoss_kwargs."""
    crit = cfg.get("criterion")
    if not isinstance(crit, dict) or crit.get("name") != "OHEM":
        return None
    return ProbOhemCrossEntropy2d(**(crit.get("kwargs") or {}))


def celoss_kwargs(cfg, num_classes):
    """(label_smoothing, weight) of cfg['criterion'] = dict(name='CELoss', kwargs=...): the two arguments of the reference's
    nn.CrossEntropyLoss(**cfg['criterion']['kwargs']) (semivl.py:142-143, supervised.py:230-231) that change the labelled
    loss's arithmetic.  `label_smoothing` must be a real number in [0, 1] (torch's own rule); `weight` a list, tuple, numpy
    array or tensor of `num_classes` numbers, returned as a contiguous fp32 tensor (a tensor already on a GPU stays there),
    or None.  Every other key (`ignore_index`, `reduction`, ...) is not read, as before.  A missing criterion, 'OHEM'
    (ProbOhemCrossEntropy2d has no such arguments) and every other name give (0.0, None)."""
    crit = cfg.get("criterion")
    if not isinstance(crit, dict) or crit.get("name") != "CELoss":
        return 0.0, None
    kw = crit.get("kwargs") or {}
    eps = kw.get("label_smoothing", 0.0)
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not 0.0 <= float(eps) <= 1.0:
        raise ValueError(f"criterion kwargs: label_smoothing must be a real number between 0.0 and 1.0. Got: {eps!r}")
    weight = kw.get("weight")
    if weight is not None:
        if not isinstance(weight, torch.Tensor):
            weight = torch.as_tensor(np.asarray(weight, dtype=np.float64))
        weight = weight.detach().to(torch.float32).contiguous()
        # (num_classes None: a model that does not say; the kernels' wrappers then check the length against the logits)
        if weight.dim() != 1 or (num_classes is not None and weight.numel() != num_classes):
            raise ValueError(f"criterion kwargs: weight has {weight.numel()} entries (shape {tuple(weight.shape)}), expected "
                             f"{num_classes}: one number for each class")
    return float(eps), weight


def _celoss_weight_on(model, weight, dev):
    """The class weights of celoss_kwargs on `dev`: copied once and kept on the model (ops.StreamCached, like
    renormalize_img_for_clip's statistics), so that a step makes no host-to-device copy and no sync."""
    if weight is None or weight.device == dev:
        return weight
    cache = getattr(model, "_dev_cache", None)
    if not isinstance(cache, dict):
        cache = model.__dict__.setdefault("_celoss_dev_cache", {})
    key = ("celoss_weight", str(dev), tuple(weight.tolist()))
    if key not in cache:
        cache[key] = ops.StreamCached(weight.to(dev))
    return cache[key].get()


# ------------------------------------------------------------------------------------------------ the step's streams
_SIDE = {}     # device -> second stream for the gradient-free passes of the step


def _side_stream(dev):      # created by whoever asks first, create_step_streams or a step
    if dev not in _SIDE:
        _SIDE[dev] = torch.cuda.Stream(dev)
    return _SIDE[dev]


def create_step_streams(dev):
    """Create every stream a training step uses on `dev` NOW (the gradient-free passes' second stream, the weight-gradient
    stream when it is enabled, and the library's helper streams of both and of the current stream) instead of lazily inside
    the first step.  The HIP runtime assigns streams to its GPU_MAX_HW_QUEUES hardware queues in creation order and
    serialises streams that share a queue: creating the step's streams first, and only then a communicator's,
    makes that map the same in every process -- GradAllReducer calls this before it creates its communication stream."""
    dev = torch.device(dev)
    if dev.type != "cuda":
        return []
    from . import lib as L
    out = [torch.cuda.current_stream(dev), _side_stream(dev)]
    if ops.WGRAD_STREAM:
        out.append(ops._wg_stream(dev))
    with torch.cuda.device(dev):
        for s_ in out:
            L.check(L.load().svl_stream_prepare(s_.cuda_stream), "svl_stream_prepare")
    return out


def step_helper_streams(streams):
    """The library's helper streams of `streams` (ragged-row GEMM parts, the attention's leftover-row kernels run there) as
    torch ExternalStreams: the communication stream must not share a hardware queue with them either."""
    import ctypes
    from . import lib as L
    out = []
    for s_ in streams:
        h_ = ctypes.c_void_p()
        with torch.cuda.device(s_.device):
            L.check(L.load().svl_stream_helper(s_.cuda_stream, ctypes.byref(h_)), "svl_stream_helper")
        if h_.value:
            out.append(torch.cuda.ExternalStream(h_.value, device=s_.device))
    return out


# ------------------------------------------------------------------------------------------------ the two public steps
LOSS_NAMES = ("loss", "loss_x", "loss_s1", "loss_s2", "loss_fp", "loss_mc_s1", "loss_mc_s2", "loss_mc_fp")

# The decode head's attributes a step overrides from cfg and _step_scope puts back when the step ends.  The two steps differ
# in ONE attribute: `act_limit_bytes` (set by _plan_head in both) is restored after the supervised step and stays on the head
# after the semivl step, where a later grad-enabled decode reads it.  Inherited behaviour, recorded here and kept exactly:
# the semivl step always left it (every such decode then works under the limit of the last step's `act_mem_fraction`), the
# supervised step was written with the restore.  Making them alike changes what such a decode does and is not done here.
_HEAD_RESTORE_SEMIVL = ("remat", "chunk_class_images")
_HEAD_RESTORE_SUPERVISED = _HEAD_RESTORE_SEMIVL + ("act_limit_bytes",)


def _refuse_untrainable_head(model, step):
    """A head that declares `trainable = False` (MaskClip2Head; the reference's forward_train raises, maskclip2_head.py:35-36)
    is refused before the step touches the model, the optimizer or the batch."""
    head = getattr(model, "decode_head", None)
    if head is not None and getattr(head, "trainable", True) is False:
        raise ValueError(f"{step}: the decode head {type(head).__name__} is not trainable (zero-shot MaskCLIP has no training "
                         f"step; evaluate it with evaluate / tools.eval)")


@contextlib.contextmanager
def _step_scope(model, head_attrs):
    """The per-step overrides of a training step (ops.WGRAD_STREAM, the decode head's `head_attrs` and its per-step memory
    plan) are undone when the block ends -- also when it raises."""
    head = getattr(model, "decode_head", None)
    keep_wg = ops.WGRAD_STREAM
    keep_head = {a_: getattr(head, a_) for a_ in head_attrs if head is not None and hasattr(head, a_)}
    try:
        yield
    finally:
        ops.WGRAD_STREAM = keep_wg
        if head is not None:
            head._bwd_ranges = None
            # (a record for tests / logs: the level this step decided on; getattr: a step that raised before the memory plan
            # was set up -- or a decode head that is not a VLGHead -- must not replace the original exception)
            head.last_remat_step = getattr(head, "_remat_step", None)
            head._remat_step = None
            head._live_class_images = None
            for a_, v_ in keep_head.items():
                setattr(head, a_, v_)


def semivl_train_step(model, batch, iters, total_iters, cfg, optimizer=None, reducer=None, fp_masks=None,
                      return_aux=False, teacher=None, monitor=None, panel=None):
    """One iteration of semivl.py:223-328 (see _semivl_train_step for the body).  Per-step overrides taken from `cfg`
    (`wgrad_stream`, `overlap_streams`, `head_remat`, `head_chunk_class_images`) and the decode head's per-step memory
    plan are undone when the step ends -- also when it raises -- so that a later grad-enabled decode outside a training
    step (validation with gradients, a test, another batch size) never inherits a stale decision.

    The MaskCLIP guidance follows the reference's own test, `cfg['maskclip_consistency_lambda'] != 0` (semivl.py:158,234,
    283,296,309): a scalar 0 / 0.0 switches it off -- no frozen-encoder forward, no guidance maps, `mc = NULL` in the three
    unlabelled cross entropies, `losses[5:8]` exactly 0, `aux['mclip']` / `aux['mclip_other']` None -- whether or not the
    model has a `clip_encoder`; a list or tuple (also [0, 0]) or a missing key keeps it on, and then a model built with
    `clip_encoder=None` is refused with a ValueError before the step touches anything.

    `teacher` (an ema.EmaTeacher over `model` and `optimizer`, or None: the step as it always was): the mean teacher.  With
    teacher.labels the pseudo-labels of both weak views come from ONE gradient-free pass of teacher.model over
    cat(img_w, img_w_other) -- on the step's second stream for every model, a conv_encoder or a BatchNorm head included:
    the teacher reads its own running statistics, not the ones the train-mode forwards write.  The student's forwards are
    launched exactly as without a teacher; its pred_w is simply no longer the source of labels.  forward_maskclip stays on
    the student, whose encoder is frozen and shared.  After optimizer.step() the teacher's BatchNorm statistics follow
    (teacher.update_buffers(optimizer.ema_decay_at(optimizer.step_count)), one launch); its weights are the optimizer's EMA
    arena and need nothing.  With return_aux, mask_w / conf_w / mask_w_other are the teacher's, pred_w_other is the
    teacher's logits for img_w_other, pred_w stays the student's and pred_w_teacher is added.  With teacher.labels False the
    step only maintains the teacher.

    `monitor` (a monitor.PseudoLabelMeter, or None: the step launches exactly what it launches without one): the label maps
    of the weak view the step trains on -- mask_w, conf_w, the guidance when the step is guided, the teacher's maps when it
    supplies the labels -- are counted against batch['ignore_mask'] and, when the batch carries it, the held-back annotation
    batch['mask_u'] (monitor.update, one launch on the main stream after the label join), and the step's loss vector is
    added to the meter's sum (monitor.add_losses, one launch).  Neither reads anything back; `aux` gets no new key.

    `panel` (a panel.StepPanel, or None: the step launches and returns exactly what it does without one): what the reference
    plots once per epoch (semivl.py:375-397) is rendered into the panel's canvas after the losses, on the main stream -- the
    four images after CutMix, the label maps of the logits of x, s1, s2 and w_fp through the step's own _smax(pred, s.up)
    (the kernel that makes mask_w: a tile shows what the step would train on), mask_x, the two mixed pseudo-label maps and
    mask_w, and when guided the two mixed guidance maps and mclip.  Nothing the step computes reads the canvas."""
    _refuse_untrainable_head(model, "semivl_train_step")
    with _step_scope(model, _HEAD_RESTORE_SEMIVL):
        return _semivl_train_step(model, batch, iters, total_iters, cfg, optimizer, reducer, fp_masks, return_aux,
                                  teacher, monitor, panel)


def supervised_train_step(model, batch, iters, total_iters, cfg, optimizer=None, reducer=None, return_aux=False,
                          teacher=None):
    """One iteration of the labelled-only baseline, third_party/unimatch/supervised.py:268-301 (method 'supervised').
    `batch`: dict with `img_x` [B, 3, S, S] fp32 and `mask_x` [B, S, S] int64 on the GPU (data.LabeledLoader,
    synthetic_batch).  model.train(), ONE forward on img_x, criterion from supervised_criterion(cfg) (cross entropy with
    ignore 255, or OHEM relabelling on the device followed by the same cross entropy), loss = the plain mean over the kept
    pixels (weight 1, not the 1/2 of semivl.py:319); its gradient scale 1 / count is formed on the device
    (svl_inv_count_f32): no host sync.  CELoss kwargs `label_smoothing` / `weight` (celoss_kwargs) select the
    cross-entropy kernels' label-smoothing / class-weight variant: torch's weighted, smoothed mean, its scale 1 / D with
    D = the sum of weight[target] over the labelled pixels, also formed on the device.  Then optimizer.zero_grad(), backward (reducer.begin() / finish() around it),
    optimizer.step() and optimizer.poly_lr(iters, total_iters) -- supervised.py:294-300 has no warm-up and no
    scheduler_max_iters, so cfg's `warmup_iters` / `scheduler_max_iters` are ignored here.
    Returns the device tensor `loss` [1]; with `return_aux` also dict(pred_x [B, N, S, S], dlogits, mask_x_ohem (None
    without OHEM), upsample_in_loss; `grad_stats` too when the optimizer clips the gradient norm).  Per-step overrides taken from `cfg` (`wgrad_stream`, `overlap_streams`,
    `head_remat`, `head_chunk_class_images`, `act_mem_fraction`) are set up for one decode of B samples and undone when
    the step ends -- also when it raises -- as in semivl_train_step.  `teacher` (ema.EmaTeacher or None): there are no
    pseudo-labels here, the step only maintains it -- teacher.update_buffers after optimizer.step()."""
    _refuse_untrainable_head(model, "supervised_train_step")
    with _step_scope(model, _HEAD_RESTORE_SUPERVISED):
        return _supervised_train_step(model, batch, iters, total_iters, cfg, optimizer, reducer, return_aux, teacher)


# ------------------------------------------------------------------------------------------------ what both steps do
def _celoss_setup(model, eps_weight, dev):
    """celoss_kwargs' (label_smoothing, weight) -> (weight on `dev` or None, the labelled CE launch's kwargs: {} = plain path)."""
    eps, cw = eps_weight
    cw = _celoss_weight_on(model, cw, dev)
    return cw, (dict(label_smoothing=eps, class_weight=cw) if (eps != 0.0 or cw is not None) else {})


# The weight-gradient stream is a process-wide switch (ops.WGRAD_STREAM: environment, multi_rank_defaults() or the caller);
# a step only overrides it when its cfg says so explicitly (_step_scope puts it back)
def _stream_override(cfg):
    if "wgrad_stream" in cfg:
        ops.WGRAD_STREAM = bool(cfg["wgrad_stream"])
    elif not cfg.get("overlap_streams", True):
        ops.WGRAD_STREAM = False


def _head_res(model, img, cfg, lsw=False):
    """`up` = (H, W, align_corners) when the logits can stay at the head's resolution (the bilinear resize to the crop is then
    evaluated inside the softmax-max / cross-entropy kernels), else None: models without the option, geometries the kernels
    do not take, cfg['fuse_upsample_loss'] / SVL_NO_UP_LOSS.  `lsw`: the labelled cross entropy runs its label-smoothing /
    class-weight variant, whose own geometry query (ops.ce_up_lsw_ok) must allow it too."""
    if img.is_cuda and cfg.get("fuse_upsample_loss", ops.UP_LOSS) and hasattr(model, "head_res_size"):
        hs = model.head_res_size(tuple(img.shape[2:]))
        geom = (img.shape[0], model.num_classes, hs[0], hs[1], img.shape[2], img.shape[3], model.align_corners) if hs else None
        if hs is not None and ops.ce_up_ok(*geom) and (not lsw or ops.ce_up_lsw_ok(*geom)):
            return (int(img.shape[2]), int(img.shape[3]), bool(model.align_corners))
    return None


# The grad-carrying decodes of a step keep `live_samples` samples' activations until backward: the head decides ONCE per step
# whether they fit or are re-materialised (model/vlg_head.py::_remat_decision) -- activations are kept while the allocation
# stays under cfg's `act_mem_fraction` of the device, the others are recomputed in backward.
def _plan_head(head, cfg, live_samples, bwd_ranges, img):
    """The decode head's per-step memory plan.  `bwd_ranges`: {decoded batch: [(first, last) samples with a gradient]} or None."""
    if head is None:
        return
    head._bwd_ranges = bwd_ranges
    head._live_class_images = live_samples * head.num_classes
    head._remat_step = {}
    if "head_remat" in cfg:
        head.remat = cfg["head_remat"]
    if cfg.get("head_chunk_class_images"):
        head.chunk_class_images = int(cfg["head_chunk_class_images"])
    frac = cfg.get("act_mem_fraction", 0.70)
    head.act_limit_bytes = (None if frac is None or not img.is_cuda else
                            int(frac * torch.cuda.get_device_properties(img.device).total_memory))


def _cat2(a, b):
    """torch.cat((a, b)) along dim 0 with the library's copy kernel; int64 maps are copied as pairs of fp32 words."""
    out = ops.empty(a.shape[0] + b.shape[0], *a.shape[1:], dtype=a.dtype, device=a.device)
    fa, fb, fo = (t_.view(torch.float32).view(-1) for t_ in (a.contiguous(), b.contiguous(), out))
    ops.eltwise(4, fa, None, out=fo[:fa.numel()])
    ops.eltwise(4, fb, None, out=fo[fa.numel():])
    return out


def _smax(pred, up):
    return ops.softmax_max_up(pred, *up) if up is not None else ops.softmax_max(pred)


def _ce(up, pred, *a_, **kw):       # the fused cross entropy on logits at the head's resolution (`up`) or on resized ones
    if up is not None:
        return ops.ce_up_fused(pred, up[0], up[1], up[2], *a_, **kw)
    return ops.ce_fused(pred, *a_, **kw)


def _full_res(pred, up):    # (return_aux only) the resized logits the fused kernels never write
    if up is None:
        return pred
    pred = pred.contiguous()
    return ops.bilinear_planes_fwd(pred, pred.shape[2], pred.shape[3], up[2], up[0], up[1])


def _backward_and_update(outputs, grads, optimizer, reducer, teacher, iters, max_iters, **warmup):
    """The tail of both steps: backward, all-reduce, optimizer.step, poly_lr(iters, max_iters, **warmup), teacher statistics."""
    if optimizer is not None:
        optimizer.zero_grad()
    torch.autograd.backward(outputs, grads)
    if reducer is not None:
        reducer.finish()    # folds autograd-delivered grads, flushes / waits for the overlapped all-reduce buckets
    if optimizer is not None:
        optimizer.step()
        optimizer.poly_lr(iters, max_iters, **warmup)
        if teacher is not None:
            teacher.update_buffers(optimizer.ema_decay_at(optimizer.step_count))


def _with_grad_stats(aux, optimizer):
    """aux['grad_stats'] = the optimizer's device tensor {norm, coef, scale, non-finite flag} when it clips the gradient
    norm (ArenaOptimizer.grad_clip); without clipping aux keeps exactly its keys."""
    if getattr(optimizer, "grad_clip", None) is not None:
        aux["grad_stats"] = optimizer.grad_stats
    return aux


# ------------------------------------------------------------------------------------------------ the labelled-only step
def _supervised_train_step(model, batch, iters, total_iters, cfg, optimizer, reducer, return_aux, teacher=None):
    ohem = supervised_criterion(cfg)                     # supervised.py:222-231 (raises on what the kernels cannot do)
    img_x, mask_x = batch["img_x"], batch["mask_x"]
    B, dev = img_x.shape[0], img_x.device
    # CELoss kwargs (supervised.py:230-231): label_smoothing / weight reach the cross-entropy kernels; {} is the plain path
    cw, ce_kw = _celoss_setup(model, celoss_kwargs(cfg, getattr(model, "num_classes", None)), dev)
    _stream_override(cfg)
    _plan_head(getattr(model, "decode_head", None), cfg, B, None, img_x)   # one grad-carrying decode, every sample live
    # (the cross-entropy kernels index the label map by the logits' geometry: a map of another shape is refused here)
    if mask_x.dtype != torch.int64 or tuple(mask_x.shape) != (B,) + tuple(img_x.shape[2:]):
        raise ValueError(f"supervised_train_step: mask_x {tuple(mask_x.shape)} {mask_x.dtype} does not match img_x "
                         f"{tuple(img_x.shape)} (expected int64 [B, S, S])")
    mask_x = mask_x.contiguous()
    if reducer is not None:
        reducer.begin()
    up = _head_res(model, img_x, cfg, lsw=bool(ce_kw))
    model.train()                                        # supervised.py:268
    pred = model(img_x, **(dict(head_res=True) if up is not None else {}))     # :277
    count = ops.zeros(1, dtype=torch.int64, device=dev)
    mask_x_ohem = None
    if ohem is not None:    # criterion = OHEM: the plain CE on the relabelled map, its count as normaliser
        mask_x = mask_x_ohem = ohem.relabel(pred, mask_x, up=up, counts_out=count)
    else:
        ops.count_valid(mask_x, count)
    gscale = ops.zeros(2, device=dev)                    # {g_t, g_m}: g_m stays 0
    if cw is not None:      # torch's weighted mean: the normaliser is D = sum of w[target] over the labelled pixels
        ops.scale_from_sum(ops.class_weight_sum(mask_x, cw, ops.empty(1, dtype=torch.float64, device=dev)), 1.0, gscale)
    else:
        ops.inv_count(count, gscale)
    dlogits = torch.empty_like(pred)
    # sums[0] = {sum ce, 0, 0, #kept}; svl_semivl_loss's `loss_x` slot is sums[0][0] / sums[0][3] -- the mean, weight 1 (:279).
    # (with CELoss kwargs: {numerator, 0, 0, D}, the same quotient.)
    # The other three branches do not exist here: their rows are zero and their slots of `out` are never read.
    sums = ops.zeros(4, 4, dtype=torch.float64, device=dev)
    _ce(up, pred.detach(), mask_x, True, dlogits=dlogits, gscale=gscale, sums_out=sums[0], **ce_kw)
    out = ops.empty(8, device=dev)
    ops.semivl_loss(sums, float(mask_x.numel()), 0.0, out)
    loss = out[1:2]
    # supervised.py:285-287, then :294-300: lr * (1 - iters / total_iters) ** 0.9, nothing else
    _backward_and_update([pred], [dlogits], optimizer, reducer, teacher, iters, total_iters)
    if return_aux:
        aux = dict(pred_x=_full_res(pred.detach(), up), dlogits=dlogits, mask_x_ohem=mask_x_ohem,
                   upsample_in_loss=up is not None)
        return loss, _with_grad_stats(aux, optimizer)
    return loss


# ------------------------------------------------------------------------------------------------ the semivl step
def _semivl_train_step(model, batch, iters, total_iters, cfg, optimizer=None, reducer=None, fp_masks=None,
                       return_aux=False, teacher=None, monitor=None, panel=None):
    """One iteration of semivl.py:223-328 (method 'semivl', CELoss(ignore 255) or OHEM (cfg['criterion']) / CELoss; conf_mode 'pixelwise' /
    'pixelavg' / 'pixelratio', train_utils.py:30-49; mcc_loss_reduce 'mean_all' / 'mean_valid' / 'mean', semivl.py:52-58).  `batch`: the 12 step tensors on the GPU.  No host syncs: the
    returned `losses` is a device float[8] (LOSS_NAMES order).  CELoss kwargs `label_smoothing` / `weight` (celoss_kwargs)
    change the labelled launch only: `losses[1]` is torch's smoothed / weighted loss_x and enters `losses[0]` as before.
    The phases below pass tensors as arguments and results; `s` holds the step's decisions (no tensors).
    """
    # 1. everything that can refuse the cfg comes first: nothing has been touched when it raises
    s = _semivl_cfg(cfg, iters, total_iters, getattr(model, "num_classes", None),
                    getattr(model, "clip_encoder", None) is not None)
    b, img_x = batch, batch["img_x"]
    cw_x, ce_kw_x = _celoss_setup(model, s.celoss, img_x.device)
    # CutMix images (in place, like the reference)
    cutmix_img_(b["img_s1"], b["img_s1_other"], b["mix1"])
    cutmix_img_(b["img_s2"], b["img_s2_other"], b["mix2"])
    head = getattr(model, "decode_head", None)
    if head is not None:
        head._bwd_ranges = None
    if reducer is not None:
        reducer.begin()
    _stream_override(cfg)
    s.B, s.return_aux, s.use_t = img_x.shape[0], return_aux, teacher is not None and teacher.labels
    # (a decode head with BatchNorm -- the DeepLabV3+ head: `has_batchnorm`)
    s.head_bn = bool(getattr(head, "has_batchnorm", False))
    # The logits stay at the head's resolution (round 5): the bilinear resize to the crop (vlg_head.py:247, builder.py:93-97)
    # is evaluated inside the softmax-max / cross-entropy kernels and the gradient comes back at the head's resolution --
    # the [B, N, H, W] tensors and the two resize passes do not exist.  `up` = (H, W, align_corners) or None (the resized
    # tensors as before).  (The labelled launch's label-smoothing / class-weight variant has its own geometry query: where it
    # refuses, the whole step runs on the resized tensors.)
    s.up = _head_res(model, img_x, cfg, lsw=bool(ce_kw_x))
    s.fwd_kw = dict(head_res=True) if s.up is not None else {}
    lab = _label_pass(model, teacher, b, cfg, s)                                             # 2. (forks to the second stream)
    preds4, preds_s = _student_forwards(model, b, cfg, fp_masks, s)                          # 3.
    _join_labels(lab, preds4[:s.B], s)                                                       # 4. (joins it)
    if monitor is not None:     # the maps the step trains on, counted on the main stream; nothing is read back
        monitor.update(lab.mask_w, lab.conf_w, b["ignore_mask"], cfg["conf_thresh"],
                       mclip=lab.mclip if s.guided else None, mask_u=b.get("mask_u"))
    mix = _cutmix_labels(lab, b, s.guided)                                                   # 5.
    # 6. / 7.: normalisers -> per-branch gradient scales, then the four fused cross entropies and the loss vector
    norm = _normalisers(preds4[s.B:2 * s.B], b["mask_x"], lab, b["ignore_mask"], mix, cw_x, cfg, s)
    losses, dl4, dls = _branch_losses(preds4, preds_s, lab, b["ignore_mask"], mix, norm, ce_kw_x, cfg, s)
    if monitor is not None:
        monitor.add_losses(losses)
    if panel is not None:
        _panel_capture(panel, iters, b, preds4, preds_s, lab, mix, s)
    if cfg.get("step_barrier", False) and dist.is_initialized() and dist.get_world_size() > 1:
        # semivl.py:325: the reference synchronises all ranks before every backward.  It orders nothing the gradient
        # all-reduce does not order already, so it is off by default; the flag restores the reference's
        # lock-step pacing (useful when per-rank logging / timing is compared against the reference's).
        dist.barrier()
    try:    # 8. backward (+ all-reduce) + optimizer
        _backward_and_update([preds4, preds_s], [dl4, dls], optimizer, reducer, teacher, iters,
                             cfg.get("scheduler_max_iters", total_iters), warmup_iters=cfg.get("warmup_iters", 0),
                             warmup_ratio=cfg.get("warmup_ratio", 1e-6))
    finally:
        if head is not None:
            head._bwd_ranges = None
    if return_aux:      # 9.
        return losses, _with_grad_stats(_semivl_aux(lab, preds4, preds_s, dl4, dls, norm.mask_x_ohem, s), optimizer)
    return losses


def _semivl_cfg(cfg, iters, total_iters, num_classes, has_clip_encoder):
    """Phase 1, host code only, all that can refuse the cfg: conf_mode, mcc_reduce, ohem, celoss, lam (at `iters`), guided."""
    conf_mode = cfg.get("conf_mode", "pixelwise")
    mcc_reduce = cfg.get("mcc_loss_reduce", "mean_all")
    if conf_mode not in ("pixelwise", "pixelavg", "pixelratio"):
        raise ValueError(conf_mode)                      # train_utils.py:47-48
    if mcc_reduce not in ("mean_all", "mean_valid", "mean"):
        raise ValueError(mcc_reduce)                     # semivl.py:161-162
    ohem = supervised_criterion(cfg)                     # semivl.py:142-149 (raises on what the kernels cannot do)
    # CELoss kwargs (semivl.py:142-143): label_smoothing / weight change the labelled launch only; (0.0, None) is the plain path
    celoss = celoss_kwargs(cfg, num_classes)
    lam_cfg = cfg.get("maskclip_consistency_lambda", [0.1, 0])
    if isinstance(lam_cfg, (list, tuple)):
        prog = iters / total_iters
        lam = lam_cfg[0] * (1 - prog) + lam_cfg[1] * prog
    else:
        lam = lam_cfg
    # semivl.py:158: the reference builds the guidance criterion, runs the frozen encoder (:234) and adds the three guidance
    # terms (:283,296,309) only `if cfg['maskclip_consistency_lambda'] != 0` -- a scalar 0 switches all of it off, a list
    # (even [0, 0]) or a missing key keeps it on
    guided = lam_cfg != 0
    if not guided:
        lam = 0.0
    elif not has_clip_encoder:
        raise ValueError(f"semivl_train_step: maskclip_consistency_lambda={lam_cfg!r} asks for the MaskCLIP guidance but the "
                         f"model was built with clip_encoder=None; set maskclip_consistency_lambda=0 (experiment 41's rows) "
                         f"or build the model with a clip_encoder")
    return SimpleNamespace(conf_mode=conf_mode, mcc_reduce=mcc_reduce, ohem=ohem, celoss=celoss, lam=lam, guided=guided)


def _label_pass(model, teacher, b, cfg, s):
    """Phase 2, gradient-free: pseudo-labels of img_w_other (student) or of both weak views (teacher) and the guidance maps.
    Sets s.main / s.side / s.pl_side: the caller's stream, the guidance's and the pseudo-label pass's (None = the caller's)."""
    B, dev, on_gpu = s.B, b["img_x"].device, b["img_x"].is_cuda
    # pseudo labels + MaskCLIP guidance (model.eval(): the side encoder's BatchNorm uses its running statistics here,
    # semivl.py:228-244; nothing else on the path depends on the mode).  Both passes are gradient-free and independent of
    # the two student forwards below: they are enqueued on a second stream (event-forked from / joined back into the
    # caller's stream), so their kernels fill the partial last rounds of the student's grids instead of queueing behind
    # them.  With a conv_encoder only the frozen-CLIP guidance moves over: the pseudo-label pass reads, in eval mode, the
    # BatchNorm running statistics that the train-mode forwards update, so it stays in program order on the main stream.
    # (the same holds for a decode head with BatchNorm: s.head_bn)
    side = (_side_stream(dev) if on_gpu and cfg.get("overlap_streams", True) and not os.environ.get("SVL_NO_SIDE_STREAM")
            else None)
    s.main = torch.cuda.current_stream(dev) if on_gpu else None
    # (a mean teacher that supplies the labels reads its OWN running statistics: its pass goes to the second stream for
    # every model)
    pl_side = side if (s.use_t or (getattr(model, "conv_encoder", None) is None and not s.head_bn)) else None
    if not s.guided and pl_side is None:
        side = None         # nothing would run there: no fork, no join
    s.side, s.pl_side = side, pl_side
    lab = SimpleNamespace(mclip_all=None, mclip=None, mclip_other=None)
    model.eval()
    if side is not None:
        side.wait_stream(s.main)
    img_ww = None
    # (torch.cuda.stream(None) changes nothing: the pass stays on the caller's stream.  lab.pred: the pass's logits, kept for
    # aux only; lab.side_maps: what _join_labels hands over to the main stream)
    with torch.no_grad(), torch.cuda.stream(pl_side):
        if s.use_t:     # ONE pass of the averaged weights over both weak views: [w, w_other]
            img_ww = _cat2(b["img_w"], b["img_w_other"])
            lab.pred = teacher.model(img_ww, **s.fwd_kw)
            conf_t, mask_t = lab.side_maps = tuple(_smax(lab.pred, s.up))
            lab.conf_w, lab.mask_w, lab.conf_w_other, lab.mask_w_other = conf_t[:B], mask_t[:B], conf_t[B:], mask_t[B:]
        else:
            lab.pred = model(b["img_w_other"], **s.fwd_kw)
            lab.conf_w_other, lab.mask_w_other = lab.side_maps = tuple(_smax(lab.pred, s.up))
        if not s.return_aux:
            lab.pred = None
    if s.guided:
        with torch.no_grad(), torch.cuda.stream(side):
            if img_ww is None or side is not pl_side:    # (reused only when both passes share a stream)
                img_ww = _cat2(b["img_w"], b["img_w_other"])
            lab.mclip_all = model.forward_maskclip(img_ww, cfg.get("mcc_conf_thresh", 0.9),
                                                   ignore_mask=_cat2(b["ignore_mask"], b["ignore_mask_other"]))
            lab.mclip, lab.mclip_other = lab.mclip_all[:B], lab.mclip_all[B:]
    model.train()          # semivl.py:246: unconditionally back to train mode
    return lab


def _wx(m_, B):     # rows in the reference's [x, w] order -> the step's [w, x]
    return torch.cat((m_[B:2 * B], m_[:B]))


@contextlib.contextmanager
def _hooks_wx(backbone, B):
    """Injected prompt-dropout / stochastic-depth masks of the backbone come in the reference's [x, w] row order too: inside
    the block both hooks hand them over as [w, x]; the hooks are put back when it ends, also when the forward raises."""
    keep = {n_: getattr(backbone, n_) for n_ in ("prompt_mask_hook", "drop_path_hook") if getattr(backbone, n_, None) is not None}
    for n_, h_ in keep.items():
        def swapped(*a_, hook=h_):
            m_ = hook(*a_)
            return None if m_ is None else _wx(m_, B)
        setattr(backbone, n_, swapped)
    try:
        yield
    finally:
        for n_, h_ in keep.items():
            setattr(backbone, n_, h_)


def _student_forwards(model, b, cfg, fp_masks, s):
    """Phase 3: the grad-carrying forwards -> preds4 over [w, x, w_fp] (BatchNorm head: + x_fp), preds_s over [s1, s2]."""
    B = s.B
    # the feature-perturbed copy of the labeled half (pred_x_fp) is never read by the step (semivl.py:247): only the
    # unlabeled half is perturbed and decoded.  The batch is ordered [w, x] (the reference: [x, w]; every op is
    # per-sample or a permutation-invariant batch statistic) so that the decoded batch is [w, x, w_fp]: the two
    # gradient-carrying thirds are CONTIGUOUS and the head's backward runs once on 2B samples (full grid rounds)
    # instead of twice on B.
    if fp_masks is not None:   # injected masks come in the reference's [x, w] row order
        fp_masks = [_wx(m_, B) for m_ in fp_masks]
    # pred_w is detached (semivl.py:251) -> exactly-zero dlogits: the head decodes those samples without keeping
    # activations and its backward skips them (results identical).  Both grad-carrying decodes of the step ([x, w_fp] here,
    # [s1, s2] below) keep activations until backward: 4 B live samples.
    _plan_head(getattr(model, "decode_head", None), cfg, 4 * B, {3 * B: [(B, 3 * B)]}, b["img_x"])
    # A head with BatchNorm decodes all 4 B samples, [w, x, w_fp, x_fp]: with batch statistics x_fp enters every mean and
    # variance of the reference's need_fp forward (cat((f, dropout2d(f))) over [x, w], builder.py:78-89), so it cannot be
    # left out; its dlogits are zero like pred_w's, and backward runs on the whole batch (the statistics terms carry
    # gradient into those rows).
    fp_kw = {} if s.head_bn else dict(fp_range=(0, B))
    with _hooks_wx(getattr(model, "backbone", None), B):
        preds4 = model(_cat2(b["img_w"], b["img_x"]), need_fp=True, fp_masks=fp_masks, split_fp=False, **fp_kw, **s.fwd_kw)
    preds_s = model(_cat2(b["img_s1"], b["img_s2"]), **s.fwd_kw)                             # [s1, s2]
    return preds4, preds_s


def _join_labels(lab, pred_w, s):
    """Phase 4: the student's own pseudo-labels; then the join: the second stream's label maps are consumed from here on."""
    if not s.use_t:
        lab.conf_w, lab.mask_w = _smax(pred_w.detach(), s.up)
    if s.side is not None:
        s.main.wait_stream(s.side)
        for t_ in (lab.side_maps if s.pl_side is not None else ()) + ((lab.mclip_all,) if s.guided else ()):
            t_.record_stream(s.main)


def _cutmix_labels(lab, b, guided):
    """Phase 5: CutMix of the label maps -> (mask, conf, ignore, guidance) pairs for the branches (s1, s2)."""
    def both(t_, other):
        return cutmix_mask(t_, other, b["mix1"]), cutmix_mask(t_, other, b["mix2"])
    # (not guided: the cross-entropy kernels take mc == NULL, their guidance sums stay 0)
    return SimpleNamespace(mw=both(lab.mask_w, lab.mask_w_other), cw=both(lab.conf_w, lab.conf_w_other),
                           ig=both(b["ignore_mask"], b["ignore_mask_other"]),
                           mc=both(lab.mclip, lab.mclip_other) if guided else (None, None))


def _normalisers(pred_x, mask_x, lab, ign, mix, cw_x, cfg, s):
    """Phase 6: the normalisers of the branches (x, s1, s2, fp) -> their gradient scales, on the device; mask_x as CE reads it."""
    dev, ohem = ign.device, s.ohem
    branches = ((mix.cw[0], mix.ig[0]), (mix.cw[1], mix.ig[1]), (lab.conf_w, ign))      # (conf, ignore) of s1, s2, fp
    counts = ops.zeros(4, dtype=torch.int64, device=dev)
    mask_x_ohem = None
    if ohem is not None:   # semivl.py:267 with criterion_l = OHEM: the plain CE on the relabelled map, its count as normaliser
        mask_x = mask_x_ohem = ohem.relabel(pred_x, mask_x, up=s.up, counts_out=counts[0:1])
    for i, m_ in enumerate((mask_x, mix.ig[0], mix.ig[1], ign)):
        if i > 0 or ohem is None:
            ops.count_valid(m_, counts[i:i + 1])
    numel_u = float(ign.numel())
    gscale = ops.empty(4, 2, device=dev)
    factors = None
    if s.conf_mode == "pixelavg":  # train_utils.py:43-46: (sum of the WHOLE CE map) * sum_b mean_valid(conf_b) / #valid
        factors = ops.empty(3, dtype=torch.float64, device=dev)
        for i, (c_, g_) in enumerate(branches):
            ops.conf_avg_factor(c_, g_, factors[i:i + 1])
    ratios = (None, None, None)
    if s.conf_mode == "pixelratio":   # train_utils.py:39-42: image b's CE map times its share of confident valid pixels
        ratios = tuple(ops.conf_ratio(c_, g_, cfg["conf_thresh"]) for c_, g_ in branches)
    mc_counts = None                # semivl.py:52-58: the guidance loss's normaliser
    if not s.guided:
        pass                        # no guidance term: no normaliser either ('mean' would count 0 labelled pixels -> 0 * x / 0)
    elif s.mcc_reduce == "mean_valid":
        mc_counts = counts[1:]
    elif s.mcc_reduce == "mean":    # nn.CrossEntropyLoss(ignore_index=255): mean over the labelled guidance pixels
        mc_counts = ops.zeros(3, dtype=torch.int64, device=dev)
        for i, m_ in enumerate(mix.mc + (lab.mclip,)):
            ops.count_valid(m_, mc_counts[i:i + 1])
    ops.semivl_gscale(counts, numel_u, s.lam, gscale, factors, mc_counts)
    if cw_x is not None:    # torch's weighted mean: g_t of the labelled branch is 0.5 / D, D = sum of w[target] (counts[0] stays)
        ops.scale_from_sum(ops.class_weight_sum(mask_x, cw_x, ops.empty(1, dtype=torch.float64, device=dev)), 0.5, gscale[0])
    return SimpleNamespace(mask_x=mask_x, mask_x_ohem=mask_x_ohem, numel_u=numel_u, gscale=gscale, factors=factors,
                           ratios=ratios, mc_counts=mc_counts)


def _branch_losses(preds4, preds_s, lab, ign, mix, norm, ce_kw_x, cfg, s):
    """Phase 7: the four fused cross entropies and svl_semivl_loss -> (losses [8], dl4, dls = the gradients of preds4, preds_s)."""
    B, up = s.B, s.up
    dl4, dls = torch.empty_like(preds4), torch.empty_like(preds_s)
    ops.fill(dl4[:B], 0.0)  # pred_w is detached (semivl.py:251)
    if s.head_bn:
        ops.fill(dl4[3 * B:], 0.0)   # pred_x_fp is never read (semivl.py:247)
    sums = ops.empty(4, 4, dtype=torch.float64, device=ign.device)
    # pixelavg and pixelratio weight the WHOLE CE map, not the confident valid pixels
    u_kw = dict(conf_thresh=cfg["conf_thresh"], all_pixels=s.conf_mode in ("pixelavg", "pixelratio"))
    _ce(up, preds4[B:2 * B].detach(), norm.mask_x, True, dlogits=dl4[B:2 * B], gscale=norm.gscale[0], sums_out=sums[0],
        **ce_kw_x)
    for i in (0, 1):        # s1, s2
        _ce(up, preds_s[i * B:(i + 1) * B].detach(), mix.mw[i], False, conf=mix.cw[i], ign=mix.ig[i], mc=mix.mc[i],
            dlogits=dls[i * B:(i + 1) * B], gscale=norm.gscale[1 + i], sums_out=sums[1 + i], img_weight=norm.ratios[i], **u_kw)
    _ce(up, preds4[2 * B:3 * B].detach(), lab.mask_w, False, conf=lab.conf_w, ign=ign, mc=lab.mclip,
        dlogits=dl4[2 * B:3 * B], gscale=norm.gscale[3], sums_out=sums[3], img_weight=norm.ratios[2], **u_kw)
    losses = ops.empty(8, device=ign.device)
    ops.semivl_loss(sums, norm.numel_u, s.lam, losses, norm.factors, norm.mc_counts)
    return losses, dl4, dls


def _panel_capture(panel, iters, b, preds4, preds_s, lab, mix, s):
    """The debug figure of semivl.py:375-397 in the reference's tile order; two _smax launches give the four prediction maps
    ([x, w_fp] are neighbours in preds4, [s1, s2] are preds_s)."""
    B = s.B
    with torch.no_grad():
        pm4 = _smax(preds4[B:3 * B].detach(), s.up)[1]
        pms = _smax(preds_s.detach(), s.up)[1]
    rows = [(pm4[:B], pms[:B], pms[B:], pm4[B:]),
            (b["mask_x"], mix.mw[0], mix.mw[1], lab.mask_w)]
    if s.guided:
        rows.append((None, mix.mc[0], mix.mc[1], lab.mclip))
    panel.capture(iters, (b["img_x"], b["img_s1"], b["img_s2"], b["img_w"]), rows)


def _semivl_aux(lab, preds4, preds_s, dl4, dls, mask_x_ohem, s):
    """Phase 9 (return_aux): label maps, full-resolution logits and the loss gradients."""
    B, up = s.B, s.up
    aux = dict(mask_w=lab.mask_w, mask_w_other=lab.mask_w_other, mclip=lab.mclip, mclip_other=lab.mclip_other,
               conf_w=lab.conf_w, pred_x=_full_res(preds4[B:2 * B].detach(), up), pred_s1=_full_res(preds_s[:B].detach(), up),
               pred_w=_full_res(preds4[:B].detach(), up),
               pred_w_other=_full_res(lab.pred[B:] if s.use_t else lab.pred, up), dl4=dl4, dls=dls,
               upsample_in_loss=up is not None, mask_x_ohem=mask_x_ohem)
    if s.use_t:
        aux["pred_w_teacher"] = _full_res(lab.pred[:B], up)
        if s.pl_side is not None:
            lab.pred.record_stream(s.main)
    return aux


# ------------------------------------------------------------------------------------------------ data parallel
class GradAllReducer:
    """Data-parallel gradient mean over the flat grad arena, overlapped with backward (replaces DDP's reducer,
    semivl.py:139-140: the reference's all-reduce buckets fire from autograd hooks inside `loss.backward()`, :327).

    One process per GPU, `torch.distributed` backend 'nccl' (= RCCL over xGMI on ROCm; 'gloo' for the CPU tests).
    The arena holds only the 31.4 M live gradients (125 MB) -- the reference's DDP also reduces the 86.8 M never-updated
    clip_encoder gradients.  It is cut at parameter boundaries into contiguous buckets of ~`bucket_mb`.
    The backward regions announce contributions through `gradsync.expect / ready`; a bucket whose parameters have all
    received every expected contribution (two per step: the [w, x, w_fp] graph and the [s1, s2] graph both reach every
    trainable tensor) is all-reduced (SUM) at once on a dedicated communication stream that is event-ordered after the
    last gradient write, so the collective runs under the remaining backward compute: the decoder's bucket under the
    second ViT backward, layers 11..3 under the layers below them.  `finish()` (after backward) folds gradients that
    arrived through torch autograd (pos_embed behind its resize), flushes whatever is left in bucket order (same order on
    every rank) and makes the compute stream wait for all collectives before the optimizer.  xGMI is point-to-point (~153 GB/s per
    link): a 25 MB bucket is ~0.3 ms on the ring, so few, large buckets; the 1/W of the mean is folded into the optimizer's
    kernel (grad_scale).  Loss normalisers stay per-rank as in the reference.
    Gradient-norm clipping (ArenaOptimizer.grad_clip) needs nothing from the reducer: optimizer.step() runs after finish(),
    on the reduced arena every rank holds alike, and forms the norm of grad_scale * g -- the norm of the averaged gradient,
    identical on every rank, as under the reference's DDP.
    With `overlap=False`, or on backends that cannot run stream-ordered collectives on GPU tensors (gloo: it stages
    through the host and stalls the launching thread), the same buckets are reduced back to back in finish()."""

    def __init__(self, optimizer, bucket_mb=25, group=None, overlap=None, world=None, collective=None, profile=False):
        """`world` / `collective`: test hooks -- a stand-in for the process group (world size and a callable
        (tensor) -> work object with .wait(), run inside the communication stream's context) so that the stream-ordered
        branch (side stream, event ordering, join in finish()) executes on a single GPU, where RCCL cannot be brought up
        with two ranks.  `profile`: HIP events around every bucket's collective and around finish()'s join."""
        self.opt, self.group = optimizer, group
        self._collective = collective
        self.profile, self._ev, self.timing = bool(profile), [], None
        self.world = world if world is not None else (dist.get_world_size(group) if dist.is_initialized() else 1)
        optimizer.grad_scale = 1.0 / self.world
        n = optimizer.g.numel()
        per = max(1, int(bucket_mb * 1024 * 1024 // 4))
        groups = getattr(optimizer, "groups", None)
        self._slot = {}          # id(param) -> bucket index
        if groups:               # cut at parameter boundaries (arena order = model.named_parameters() order)
            offs = optimizer.seg_off.tolist()
            self.buckets, start, members = [], 0, []
            for i, g_ in enumerate(groups):
                members.append(g_["param"])
                if offs[i + 1] - start >= per or i == len(groups) - 1:
                    self.buckets.append((start, offs[i + 1]))
                    for prm in members:
                        self._slot[id(prm)] = len(self.buckets) - 1
                    start, members = offs[i + 1], []
        else:                    # bare arena (tests)
            self.buckets = [(s, min(n, s + per)) for s in range(0, n, per)]
        self._members = [0] * len(self.buckets)
        for b_ in self._slot.values():
            self._members[b_] += 1
        backend = dist.get_backend(group) if (dist.is_initialized() and self.world > 1) else None
        if collective is not None:
            backend = "nccl"          # the injected collective is stream-ordered like RCCL's
        self.overlap = (backend == "nccl") if overlap is None else bool(overlap)
        self._async = backend == "nccl"
        # Where the collective's kernel runs.  ProcessGroupNCCL issues an `async_op=True` collective on a stream of ITS
        # OWN (ordered after the caller's current stream), so the hardware queue that matters is one this class never
        # sees.  Since torch 2.8 a blocking-style call (`async_op=False`) is enqueued on the CURRENT stream instead: issued
        # inside `torch.cuda.stream(self._comm)` the RCCL kernel runs on the communication stream picked below -- the one
        # whose queue was probed against the step's streams.  (`on_comm_stream=False`, or an older torch, keeps the
        # async form + a stream-level wait.)
        tv = tuple(int(x) for x in torch.__version__.split("+")[0].split(".")[:2])
        self.on_comm_stream = tv >= (2, 8) and not os.environ.get("SVL_RCCL_ASYNC_OP")
        # stream -> hardware-queue map: the step's own streams are created FIRST (deterministic map, see
        # create_step_streams), then the communication stream, and the result is probed once and kept for the bench line
        self.queue_info = None
        on_gpu = optimizer.g.is_cuda
        if on_gpu and self.world > 1:
            step_streams = create_step_streams(optimizer.g.device)
        self._comm = None
        if on_gpu and self.world > 1 and not os.environ.get("SVL_NO_QUEUE_PROBE"):
            # The communication stream is PICKED, not taken as it comes: up to six fresh streams are probed against the
            # step's streams and the first one that shares a hardware queue with none of them is kept (the runtime's
            # stream -> queue assignment is not round-robin once library helper streams exist: with 8 queues the first
            # fresh stream landed on the main stream's queue, measured).  Blocking backends have no communication stream:
            # the same search reports what one created at this point WOULD get.
            names = ["main", "second"] + (["weight_gradient"] if len(step_streams) > 2 else [])
            helpers = step_helper_streams(step_streams)          # (round 6: the leftover-row / ragged-row launches' streams too)
            names = names + [n_ + "_helper" for n_ in names[:len(helpers)]]
            step_streams = list(step_streams) + helpers
            tried, pick, shared = [], None, None
            for _ in range(8):
                cand = torch.cuda.Stream(optimizer.g.device)
                sh_ = [n_ for n_, s_ in zip(names, step_streams) if ops.streams_share_queue(s_, cand)]
                tried.append(cand)               # (kept alive: a destroyed stream's queue slot would be handed out again)
                if pick is None or len(sh_) < len(shared):
                    pick, shared = cand, sh_
                if not sh_:
                    break
            # (the unpicked candidates are kept only until the pick is made: a destroyed stream's queue slot is handed out
            # again, which is fine once nothing else is created by this class)
            self._probed_streams = [pick]
            n_tried = len(tried)
            del tried
            if self._async:
                self._comm = pick
            self.queue_info = dict(gpu_max_hw_queues=int(os.environ.get("GPU_MAX_HW_QUEUES", "4")),
                                   comm_stream_shares_queue=bool(shared), shares_queue_with=shared,
                                   streams_probed=n_tried, weight_gradient_stream=bool(ops.WGRAD_STREAM),
                                   collective_runs_on=("the communication stream (async_op=False under torch >= 2.8)"
                                                       if self.on_comm_stream else "ProcessGroupNCCL's internal stream"),
                                   comm_stream="dedicated" if self._async else "none (blocking backend; probed a stand-in)")
        elif self._async and on_gpu:
            self._comm = torch.cuda.Stream(optimizer.g.device)
        self._reset()
        self.early_fires = 0
        if self.world > 1 and groups:
            for g_ in groups:
                g_["param"]._svl_reducer = self

    def _reset(self):
        """The per-step state: works in flight, buckets fired, complete parameters per bucket, contributions per parameter."""
        self._works, self._fired = [], set()
        self._complete = [0] * len(self.buckets)
        self._expected, self._done = {}, {}

    # ---- region hooks (gradsync.expect / gradsync.ready) ---------------------------------------------------------
    def _expect(self, prm):
        self._expected[id(prm)] = self._expected.get(id(prm), 0) + 1

    def _ready(self, prm):
        k = id(prm)
        self._done[k] = self._done.get(k, 0) + 1
        if self._done[k] == self._expected.get(k, 0):
            b_ = self._slot[k]
            self._complete[b_] += 1
            if self.overlap and self._complete[b_] == self._members[b_]:
                self.early_fires += 1           # (statistics: buckets launched from inside backward)
                self._fire(b_)

    def _fire(self, b_):
        if b_ in self._fired:
            return
        self._fired.add(b_)
        s, e = self.buckets[b_]
        g = self.opt.g[s:e]
        if self._comm is not None:
            self._comm.wait_stream(torch.cuda.current_stream())     # ordered after the last gradient write
            with torch.cuda.stream(self._comm):
                if self.profile:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(self._comm)
                if self._collective is not None:
                    w = self._collective(g)
                elif self.on_comm_stream:
                    # enqueued on the current stream = self._comm (torch >= 2.8): no work object, nothing to wait for
                    dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.group, async_op=False)
                    w = None
                else:
                    w = dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                # (async form: ProcessGroupNCCL runs the collective on its OWN stream, which only waits for the caller's; the
                # stream-level wait below orders the communication stream after the collective itself, so the events
                # around it bracket its duration, not its enqueue, and joining `_comm` joins every collective.  Only for
                # works whose wait() is stream-level: a blocking wait here would stall backward on the host.)
                if w is not None and not os.environ.get("TORCH_NCCL_BLOCKING_WAIT"):
                    w.wait()
                self._works.append(w)
                if self.profile:
                    e1.record(self._comm)
                    self._ev.append((b_, (e - s) * 4, e0, e1))
        else:
            t0 = time.perf_counter() if self.profile else 0.0
            dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.group)
            if self.profile:       # blocking collective on the compute thread (gloo dry runs): host wall time, all of it exposed
                self._ev.append((b_, (e - s) * 4, None, time.perf_counter() - t0))

    def broadcast_params(self, src=0):
        if self.world > 1 and self._collective is None:
            dist.broadcast(self.opt.p, src, group=self.group)

    def begin(self):
        """Start of a step: forget whatever a previous, aborted step left behind -- a
        backward that raised, or a grad-enabled forward that never ran its backward, would otherwise carry `expected` /
        `done` counts into this step and fire a bucket before its last contribution (or never fire it early).
        semivl_train_step calls it before the first grad-enabled forward (the forwards register their `expect`s)."""
        if self._works and self._comm is not None:
            # collectives of an aborted step may still be in flight on arena slices: the next zero_grad / gradient
            # writes on the compute stream must not overtake them
            torch.cuda.current_stream().wait_stream(self._comm)
        self._reset()

    def finish(self):
        """After backward: every gradient in the arena, every bucket reduced, compute stream ordered after them."""
        if hasattr(self.opt, "_fold_autograd_grads"):
            self.opt._fold_autograd_grads()     # e.g. pos_embed behind its bicubic resize: BEFORE its bucket is reduced
        if self.world > 1:
            for b_ in range(len(self.buckets)):
                self._fire(b_)
            if self.profile and self._comm is not None:
                j0, j1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                j0.record(torch.cuda.current_stream())
            for w in self._works:
                if w is not None:
                    w.wait()                     # stream-level wait (no host sync) for NCCL/RCCL works
            if self._comm is not None:
                torch.cuda.current_stream().wait_stream(self._comm)
            if self.profile and self._comm is not None:
                j1.record(torch.cuda.current_stream())
                self.timing = dict(events=self._ev, join=(j0, j1), early_fires=self.early_fires)
                self._ev = []
            elif self.profile:
                self.timing = dict(events=self._ev, join=None, early_fires=self.early_fires)
                self._ev = []
        self._reset()

    reduce = finish

    def timing_report(self):
        """(after a synchronize) per-bucket collective time on the communication stream and the part of the step the
        compute stream spent waiting for them in finish() -- what backward did NOT hide."""
        t = self.timing
        if not t:
            return None
        if t["join"] is None:      # synchronous backend: every bucket blocks the compute thread for its whole duration
            bk = [dict(bucket=b_, mbytes=round(nb / 2 ** 20, 1), ms=round(dt * 1e3, 3)) for b_, nb, _, dt in t["events"]]
            return dict(buckets=bk, exposed_ms=round(sum(b_["ms"] for b_ in bk), 3), launched_inside_backward=t["early_fires"],
                        queues=self.queue_info,
                        note="blocking all-reduce on the compute thread (backend without stream-ordered collectives): host "
                             "wall time per bucket, all of it exposed")
        return dict(buckets=[dict(bucket=b_, mbytes=round(nb / 2 ** 20, 1), ms=round(e0.elapsed_time(e1), 3))
                             for b_, nb, e0, e1 in t["events"]],
                    exposed_ms=round(t["join"][0].elapsed_time(t["join"][1]), 3), launched_inside_backward=t["early_fires"],
                    queues=self.queue_info,
                    note="ms = HIP events around each bucket's all-reduce on the communication stream; exposed_ms = time "
                         "the compute stream waited in finish() for the collectives backward did not cover")
