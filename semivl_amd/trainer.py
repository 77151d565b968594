"""The training driver: semivl.py:166-433 (method 'semivl') and third_party/unimatch/supervised.py:239-334 (method
'supervised') on the native path -- epochs, evaluation, checkpoints, resume, logging without a per-step host sync and the
per-epoch debug panels rendered on the device (panel.py).  `tools/train.py` is its command line.

What a run leaves in `save_path`:
    config.yaml      the config as given
    train.log        the log lines (the reference's wording where it has one)
    metrics.jsonl    one JSON object per log point and per evaluation (stands in for the reference's SummaryWriter)
    latest.pth       after every epoch (cfg['trainer']['save_latest']);  best.pth  when the result improves (semivl.py:423-433)
    debug/{iters:07d}_{rank}-{b}.png     the first step of every epoch, rank 0 (cfg['trainer']['debug_panels'], 'semivl' only)

Reproducibility: at the start of every epoch Python's `random`, `numpy.random` and `torch.manual_seed` are seeded with
`epoch_seed(seed, epoch, rank)`; the augmenter draws from the first two, ops.bernoulli from torch's generator and
initial_seed().  An epoch's draws therefore do not depend on history, and a run resumed at an epoch boundary continues bit
for bit.  The model is built under epoch_seed(seed, 0, 0) on every rank.

Logging: every step's loss vector is added on the device into float64 sums and a count (svl_pl_add_losses, one launch, the
library's own: no ATen kernel enters the step's trace); at a log point ONE copy brings them over.
"""
import json
import math
import numbers
import os
import random
import time

import numpy as np
import torch
import torch.distributed as dist

from . import ops

_DEFAULTS = dict(seed=0, log_interval=100, debug_panels=True, save_latest=True, workers=4, prefetch=2)
_INT_MIN = dict(seed=0, log_interval=1, workers=1, prefetch=1)
_SEED_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ host logic
def trainer_from_cfg(cfg):
    """cfg['trainer'] (optional) -> dict(seed=0, log_interval=100, debug_panels=True, save_latest=True, workers=4,
    prefetch=2) with the given keys filled in.  seed: an int in [0, 2^31); log_interval, workers, prefetch: ints >= 1 (no
    bool); debug_panels, save_latest: bools.  A non-dict, an unknown key or a value of the wrong kind / out of range raises
    a ValueError naming the offender."""
    spec = cfg.get("trainer", {})
    if not isinstance(spec, dict):
        raise ValueError(f"trainer: expected a dict with the keys {tuple(_DEFAULTS)}, got {spec!r}")
    for k in spec:
        if k not in _DEFAULTS:
            raise ValueError(f"trainer: unknown key {k!r} (known: {tuple(_DEFAULTS)})")
    out = dict(_DEFAULTS)
    for k, v in spec.items():
        if isinstance(_DEFAULTS[k], bool):
            if not isinstance(v, bool):
                raise ValueError(f"trainer: {k} must be a bool, got {v!r}")
            out[k] = v
            continue
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"trainer: {k} must be an int, got {v!r}")
        if v < _INT_MIN[k] or (k == "seed" and v > _SEED_MAX):
            raise ValueError(f"trainer: {k} = {v!r} is out of range (>= {_INT_MIN[k]}"
                             + (f", <= {_SEED_MAX}" if k == "seed" else "") + ")")
        out[k] = int(v)
    return out


def epoch_seed(seed, epoch, rank=0):
    """The one integer mix of (seed, epoch, rank): ((seed * 1000003 + epoch) * 1009 + rank) mod 2^32 -- distinct for every
    (epoch, rank) of a run with fewer than 1009 ranks and 1000003 epochs, inside numpy's 32-bit seed range."""
    return ((int(seed) * 1000003 + int(epoch)) * 1009 + int(rank)) % (2 ** 32)


def seed_epoch(seed, epoch, rank=0):
    """Seed Python's random, numpy.random and torch (CPU generator and initial_seed()) for `epoch`; returns the seed used."""
    s = epoch_seed(seed, epoch, rank)
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)
    return s


def schedule_from_cfg(cfg, steps_per_epoch):
    """(epochs, total_iters) of semivl.py:181-187: cfg['iters'] gives epochs = ceil(iters / steps_per_epoch) (cfg['epochs']
    must then be missing or None), otherwise cfg['epochs']; total_iters = steps_per_epoch * epochs; a
    cfg['scheduler_max_iters'] below total_iters is refused like the reference's assert."""
    if steps_per_epoch < 1:
        raise ValueError(f"trainer: the loader yields {steps_per_epoch} steps per epoch (fewer samples than one batch per rank)")
    iters, epochs = cfg.get("iters"), cfg.get("epochs")
    for name, v in (("iters", iters), ("epochs", epochs)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1):
            raise ValueError(f"trainer: cfg[{name!r}] must be an int >= 1 or None, got {v!r}")
    if iters is not None:
        if epochs is not None:
            raise ValueError("trainer: cfg gives both 'iters' and 'epochs'; with 'iters' the reference wants epochs = None")
        epochs = math.ceil(iters / steps_per_epoch)
    elif epochs is None:
        raise ValueError("trainer: cfg needs 'iters' (or 'epochs')")
    total = steps_per_epoch * int(epochs)
    smax = cfg.get("scheduler_max_iters", total)
    if smax < total:
        raise ValueError(f"trainer: scheduler_max_iters = {smax} < total_iters = {total}")
    return int(epochs), total


def eval_due(epoch, epochs, every=1):
    """semivl.py:408: epoch % eval_every_n_epochs == 0 or the last epoch."""
    return epoch % every == 0 or epoch == epochs - 1


def is_log_point(iters, step_in_epoch, steps_per_epoch, log_interval):
    return iters % log_interval == 0 or step_in_epoch == steps_per_epoch - 1


def _plain(v):
    """JSON-serialisable: numpy scalars / arrays as Python numbers / lists, non-finite floats as None."""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return _plain(v.tolist())
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, numbers.Integral):
        return int(v)
    if isinstance(v, numbers.Real):
        v = float(v)
        return v if math.isfinite(v) else None
    return v


class MetricsWriter:
    """`path` gets one JSON object per `write` (a line each, appended and flushed: a resumed run continues the file)."""

    def __init__(self, path):
        self.path = str(path)
        os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)

    def write(self, kind, **values):
        rec = dict(kind=kind, **_plain(values))
        with open(self.path, "a") as f:
            f.write(json.dumps(rec, allow_nan=False) + "\n")
        return rec


def read_metrics(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


class _Log:
    def __init__(self, path, enabled):
        self.path, self.enabled = path, enabled

    def __call__(self, line):
        if not self.enabled:
            return
        print(line, flush=True)
        with open(self.path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------ device-side loss sums
class LossMeter:
    """float64 sums of k loss slots and the step count in ONE device buffer: `add` is one svl_pl_add_losses launch in step
    order, `read` the one copy to the host (the only sync) -> (sums float64 [k], steps)."""

    def __init__(self, k, device):
        self.k = int(k)
        self._buf = ops.zeros(self.k + 1, dtype=torch.float64, device=device)
        self.sum, self.steps = self._buf[:self.k], self._buf[self.k:].view(torch.int64)

    def add(self, losses):
        ops.pl_add_losses(losses.contiguous(), self.sum, self.steps)

    def read(self):
        host = self._buf.cpu()
        return host[:self.k].numpy().copy(), int(host[self.k:].view(torch.int64)[0])

    def reset(self):
        ops.fill(self._buf.view(torch.float32), 0.0)


# ------------------------------------------------------------------------------------------------ the run
def default_id_paths(cfg):
    """The reference's split files: splits/<dataset>/<split>/{labeled,unlabeled}.txt."""
    base = os.path.join("splits", str(cfg["dataset"]), str(cfg["split"]))
    return os.path.join(base, "labeled.txt"), os.path.join(base, "unlabeled.txt")


def _evaluate(model, loader, mode, cfg):
    """(mIoU, iou_class, EvalReport or None): report.evaluate_report when cfg has 'eval_report', else evaluate."""
    from .evaluate import evaluate
    from .report import evaluate_report
    if "eval_report" in cfg:
        rep = evaluate_report(model, loader, mode, cfg)
        return rep.miou, rep.iou_class, rep
    miou, iou = evaluate(model, loader, mode, cfg)
    return miou, iou, None


def train(cfg, save_path, labeled_id_path, unlabeled_id_path, resume=None, stop_after_epoch=None, device=None, on_step=None):
    """Run cfg['method'] ('semivl', the default, or 'supervised') to the end, or through epoch `stop_after_epoch`.
    `resume`: a checkpoint this function wrote (latest.pth): model, optimizer, teacher, previous_best are restored and the
    run starts at the stored epoch + 1; a stored total_iters or seed other than this cfg's raises.  `on_step(iters, losses)`
    receives every step's device loss tensor (tests).  Returns dict(best, epochs_run, report, model, optimizer, teacher)."""
    import yaml
    from .checkpoint import load_checkpoint, save_checkpoint
    from .data import GpuAugmenter, LabeledLoader, SemiDataset, StepLoader, ValLoader
    from .ema import EmaTeacher
    from .model.builder import build_model
    from .monitor import PseudoLabelMeter
    from .panel import StepPanel, palette_from_cfg
    from .train import LOSS_NAMES, GradAllReducer, optimizer_from_cfg, semivl_train_step, supervised_train_step

    # everything that can refuse the cfg comes first: nothing is built or written when it raises
    tr = trainer_from_cfg(cfg)
    method = cfg.get("method", "semivl")
    if method not in ("semivl", "supervised"):
        raise ValueError(f"trainer: method {method!r} is not supported ('semivl', 'supervised')")
    palette = palette_from_cfg(cfg)
    every = cfg.get("eval_every_n_epochs", 1)
    if isinstance(every, bool) or not isinstance(every, numbers.Integral) or every < 1:
        raise ValueError(f"trainer: eval_every_n_epochs must be an int >= 1, got {every!r}")
    eval_mode = cfg["eval_mode"]
    distributed = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if distributed else (0, 1)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    semi = method == "semivl"
    guided = semi and cfg.get("maskclip_consistency_lambda", [0.1, 0]) != 0      # the step's own test (semivl.py:158)

    aug = GpuAugmenter.from_cfg(cfg, device=device)
    loader_kw = dict(rank=rank, world=world, workers=tr["workers"], prefetch=tr["prefetch"])
    if semi:
        set_u = SemiDataset(cfg, "train_u", id_path=unlabeled_id_path)
        set_l = SemiDataset(cfg, "train_l", id_path=labeled_id_path, nsample=len(set_u.ids))
        make_loader = lambda epoch: StepLoader(set_l, set_u, aug, cfg["batch_size"], epoch=epoch, **loader_kw)
        names = LOSS_NAMES
    else:
        set_l = SemiDataset(cfg, "train_l", id_path=labeled_id_path)
        make_loader = lambda epoch: LabeledLoader(set_l, aug, cfg["batch_size"], epoch=epoch, **loader_kw)
        names = ("loss",)
    steps = len(make_loader(0))
    epochs, total_iters = schedule_from_cfg(cfg, steps)
    val_loader = ValLoader(cfg, aug, rank, world)

    with torch.cuda.device(device):
        seed_epoch(tr["seed"], 0, 0)     # the randomly initialised tensors (the decoder): the same on every rank and in every run
        model = build_model(cfg)
        model.to(device)
        optimizer = optimizer_from_cfg(model, cfg)
        teacher = EmaTeacher.from_cfg(model, optimizer, cfg)
        monitor = PseudoLabelMeter.from_cfg(cfg, cfg["nclass"], device) if semi else None
        reducer = None
        if distributed:
            reducer = GradAllReducer(optimizer)
            reducer.broadcast_params()
            if teacher is not None:
                teacher.reset()

        previous_best, start = 0.0, 0
        if resume is not None:
            ck = torch.load(resume, map_location="cpu")
            for key, mine in (("total_iters", total_iters), ("seed", tr["seed"])):
                if ck.get(key) is not None and ck[key] != mine:
                    raise ValueError(f"trainer: {resume} was written by a run with {key} = {ck[key]!r}, this cfg gives "
                                     f"{mine!r}: the resumed run would not continue the stored one")
            stored = load_checkpoint(ck, model)
            optimizer.load_state_dict(ck["optimizer"])
            if teacher is not None:
                load_checkpoint(ck, teacher.model, ema=True)
            ops.weights_changed()
            previous_best, start = float(ck.get("previous_best", 0.0)), int(stored) + 1

        main = rank == 0
        if main:
            os.makedirs(save_path, exist_ok=True)
            with open(os.path.join(save_path, "config.yaml"), "w") as f:
                yaml.dump(cfg, f)
        log = _Log(os.path.join(save_path, "train.log"), main)
        metrics = MetricsWriter(os.path.join(save_path, "metrics.jsonl")) if main else None
        panel = (StepPanel(os.path.join(save_path, "debug"), palette=palette, rank=rank)
                 if (main and semi and tr["debug_panels"]) else None)
        meter = LossMeter(len(names), device)
        extra = dict(seed=tr["seed"], total_iters=total_iters)
        if resume is not None:
            log("************ Load from checkpoint at epoch %i\n" % (start - 1))
        log(f"Train for {epochs} epochs / {total_iters} iterations.")
        report, epochs_run = None, 0
        try:
            for epoch in range(start, epochs):
                log("===========> Epoch: {:}, LR: {:.5f}, Previous best: {:.2f}".format(
                    epoch, optimizer.param_groups[0]["lr"], previous_best))
                seed_epoch(tr["seed"], epoch, rank)
                t_log, n_log = time.time(), 0
                for i, batch in enumerate(make_loader(epoch)):
                    iters = epoch * steps + i
                    if semi:
                        losses = semivl_train_step(model, batch, iters, total_iters, cfg, optimizer=optimizer, reducer=reducer,
                                                   teacher=teacher, monitor=monitor, panel=panel if i == 0 else None)
                    else:
                        losses = supervised_train_step(model, batch, iters, total_iters, cfg, optimizer=optimizer,
                                                       reducer=reducer, teacher=teacher)
                    meter.add(losses)
                    if on_step is not None:
                        on_step(iters, losses)
                    n_log += 1
                    if is_log_point(iters, i, steps, tr["log_interval"]):
                        sums, count = meter.read()          # the one copy (and the only sync) of the log point
                        meter.reset()
                        now = time.time()
                        vals = {"train/iter_time": (now - t_log) / n_log}
                        for k, name in enumerate(names):
                            if name.startswith("loss_mc") and not guided:
                                continue                    # semivl.py:357: the guidance terms are logged only when guided
                            vals["train/" + ("loss_all" if name == "loss" else name)] = float(sums[k] / count)
                        if getattr(optimizer, "grad_clip", None) is not None:
                            gs = optimizer.grad_stats.cpu().tolist()
                            vals.update({"train/grad_norm": gs[0], "train/grad_clip_coef": gs[1], "train/grad_nonfinite": gs[3]})
                        mon = None
                        if monitor is not None:            # (every rank: report() all-reduces under a process group)
                            mon = {k: v for k, v in monitor.report().items() if k != "table"}
                            monitor.reset()
                        log(f"Iters: {i} " + ", ".join(f"{k}: {v:.3f}" for k, v in vals.items()))
                        if main:
                            metrics.write("train", epoch=epoch, iters=iters, steps=count, **vals,
                                          **({"pl_monitor": mon} if mon is not None else {}))
                        t_log, n_log = time.time(), 0
                epochs_run += 1
                is_best = False
                if eval_due(epoch, epochs, every):
                    miou, iou_class, rep = _evaluate(model, val_loader, eval_mode, cfg)
                    report = dict(epoch=epoch, eval_mode=eval_mode, mIoU=miou, iou_class=np.asarray(iou_class), report=rep)
                    result = miou
                    if teacher is not None:
                        t_miou, t_iou, t_rep = _evaluate(teacher.model, val_loader, eval_mode, cfg)
                        report.update(ema_mIoU=t_miou, ema_iou_class=np.asarray(t_iou), ema_report=t_rep)
                        result = t_miou     # previous_best follows the teacher when there is one
                    for cls_idx, iou in enumerate(iou_class):
                        log("***** Evaluation ***** >>>> Class [{:}] IoU: {:.2f}".format(cls_idx, iou))
                    if rep is not None:
                        log(rep.format_table())
                    log("***** Evaluation {} ***** >>>> MeanIoU: {:.2f}\n".format(eval_mode, miou))
                    if teacher is not None:
                        log("***** Evaluation {} (ema) ***** >>>> MeanIoU: {:.2f}\n".format(eval_mode, report["ema_mIoU"]))
                    is_best = result > previous_best
                    previous_best = max(result, previous_best)
                    if main:
                        metrics.write("eval", epoch=epoch, eval_mode=eval_mode, previous_best=previous_best,
                                      **{"eval/mIoU": miou, "eval/iou_class": np.asarray(iou_class)},
                                      **({"eval/ema_mIoU": report["ema_mIoU"]} if teacher is not None else {}),
                                      **({"eval/metrics": rep.metrics()} if rep is not None else {}))
                if main and (is_best or tr["save_latest"]):
                    ema_model = teacher.model if teacher is not None else None
                    for name, wanted in (("best.pth", is_best), ("latest.pth", tr["save_latest"])):
                        if wanted:
                            save_checkpoint(os.path.join(save_path, name), model, optimizer, epoch, ema_model=ema_model,
                                            extra=dict(extra, previous_best=previous_best))
                if distributed:
                    dist.barrier()      # a resume on any rank reads the file rank 0 has just written
                if stop_after_epoch is not None and epoch >= stop_after_epoch:
                    break
        finally:
            if panel is not None:
                panel.close()
    return dict(best=previous_best, epochs_run=epochs_run, report=report, model=model, optimizer=optimizer, teacher=teacher,
                total_iters=total_iters, epochs=epochs)
