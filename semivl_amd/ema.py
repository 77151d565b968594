"""The mean teacher: a model whose trainable tensors ARE the optimizer's EMA arena.

  third_party/unimatch/eval.py:29,132-133   `--ema` evaluates checkpoint['ema_model']   -> EmaTeacher.model.state_dict()
                                            through checkpoint.save_checkpoint(..., ema_model=teacher.model)

FusedAdamW / FusedSGD keep `optimizer.ema`, a second flat arena their step kernel updates in the launch that updates the
weights (csrc/optim.hip).  EmaTeacher builds a module of the student's class and structure around it:

  * every parameter with a slot in the arena is a VIEW of `optimizer.ema` at that slot: after optimizer.step() the teacher
    is current without a launch or a copy;
  * every other parameter (frozen backbone tensors, the frozen clip_encoder, prompt_norm) and every buffer that is not a
    BatchNorm statistic is the student's own tensor object: the frozen ViT-B/16 exists once.  (clip_encoder.* and
    prompt_norm.* are registered with requires_grad=True, like the reference's, and never trained: the teacher holds the
    student's storage under a parameter of its own that asks for no gradient);
  * BatchNorm running_mean / running_var are the teacher's own (views of one flat tensor), moved towards the student's by
    update_buffers(d) in ONE launch (svl_ema_segments_f32); num_batches_tracked is copied.

The teacher's weights are rewritten by a raw kernel that bumps no version counter, and they do not require a gradient: the
weight caches of ops (weight_planes, cached_pack) would keep their packed planes for the life of the process.  Every arena
view is therefore marked `_svl_rewritten`, which gives it the per-step invalidation (ops.WEIGHT_EPOCH) trainable weights
get; the cached planes keep their ops.StreamCached hand-over, because the training step runs the teacher on its side stream.
"""
import copy

import torch

from . import ops
from .optim import arena_layout, ema_from_cfg

_BN = torch.nn.modules.batchnorm._BatchNorm


class EmaTeacher:
    """EmaTeacher(model, optimizer, buffers='ema', labels=True).  `optimizer`: a FusedAdamW / FusedSGD built with an EMA
    arena (ema_decay=, or cfg['ema'] through optimizer_from_cfg) over `model`, which is already on its device.
    `buffers`: 'ema' (the BatchNorm statistics follow the student's with the parameters' decay) or 'copy' (they ARE the
    student's after every step: d = 0).  `labels`: whether semivl_train_step takes its pseudo-labels from the teacher
    (cfg['ema']['teacher']); False only maintains it.

    `model` (the teacher) is always in eval mode and nothing on it requires a gradient; its state_dict() has the student's
    keys.  evaluate(teacher.model, loader, mode, cfg, tta=...) and predict(teacher.model, ...) take it as any model.
    The student's num_batches_tracked buffers become views of one flat int64 tensor (values kept), so that they are copied
    across by one launch as well."""

    def __init__(self, model, optimizer, buffers="ema", labels=True):
        if getattr(optimizer, "ema", None) is None:
            raise ValueError("EmaTeacher: the optimizer keeps no EMA arena (build it with ema_decay= or cfg['ema'])")
        if buffers not in ("ema", "copy"):
            raise ValueError("EmaTeacher: buffers must be 'ema' or 'copy', got %r" % (buffers,))
        if not isinstance(labels, bool):
            raise ValueError("EmaTeacher: labels must be a bool, got %r" % (labels,))
        self.student, self.optimizer, self.buffers, self.labels = model, optimizer, buffers, labels
        self._slot = {id(g_["param"]): i for i, g_ in enumerate(optimizer.groups)}
        dev = optimizer.ema.device
        # the teacher's BatchNorm statistics: one flat tensor, 16-byte aligned views
        bns = [m for m in model.modules() if isinstance(m, _BN) and m.running_mean is not None]
        sizes = [t.numel() for m in bns for t in (m.running_mean, m.running_var)]
        offs, total = arena_layout(sizes)
        self._stats = ops.zeros(total, device=dev) if total else None
        self._nbt_s = self._nbt_t = None
        if bns:
            nbt = torch.stack([m.num_batches_tracked.detach().to(dev).view(()) for m in bns])
            self._nbt_s, self._nbt_t = nbt, nbt.clone()
        self._own = {}          # id(student buffer) -> the teacher's tensor
        self._pairs = []        # (student module, buffer name, the teacher's tensor)
        for k, m in enumerate(bns):
            for j, name in enumerate(("running_mean", "running_var")):
                s = getattr(m, name)
                t = self._stats[offs[2 * k + j]:offs[2 * k + j] + s.numel()].view(s.shape)
                self._own[id(s)] = t
                self._pairs.append((m, name, t))
            m.num_batches_tracked = self._nbt_s[k]        # (a view: the module's `+= 1` lands in the flat tensor)
            self._own[id(m.num_batches_tracked)] = self._nbt_t[k]
        self._params, self._shared = {}, {}
        self.model = self._clone(model, {})
        keep = self.model

        def stay_eval(mode=True):
            return torch.nn.Module.train(keep, False)
        self.model.__dict__["train"] = stay_eval      # (Module.eval() calls self.train(False))
        self._tables = self._src_ptrs = None
        self._copy_buffers()

    @classmethod
    def from_cfg(cls, model, optimizer, cfg):
        """The teacher cfg['ema'] = dict(decay, warmup, teacher, buffers) asks for (optim.ema_from_cfg), or None without
        the key.  `optimizer` is what optimizer_from_cfg(model, cfg) built."""
        e = ema_from_cfg(cfg)
        if e is None:
            return None
        return cls(model, optimizer, buffers=e["buffers"], labels=e["teacher"])

    # ---- structure ---------------------------------------------------------------------------------------------------
    def _param(self, p):
        if p is None:
            return None
        ai = self._slot.get(id(p))
        if ai is None and not p.requires_grad:
            return p                                   # frozen: the student's own tensor object
        if ai is None:
            # clip_encoder.* / prompt_norm.*: registered as trainable like the reference's, never trained (optim._trainable).
            # The student's storage under a parameter that asks for no gradient: nothing on the teacher requires one.
            t = self._shared.get(id(p))
            if t is None:
                t = self._shared[id(p)] = torch.nn.Parameter(torch.empty(0, device=p.device), requires_grad=False)
                t.data = p.data
            return t
        t = self._params.get(id(p))
        if t is None:
            # (a Parameter whose .data is the view, like the student's: ops keys its weight caches on Parameters)
            t = torch.nn.Parameter(torch.empty(0, device=p.device), requires_grad=False)
            t.data = self.optimizer._seg(self.optimizer.ema, ai)
            t._svl_rewritten = True                    # ops.weight_planes / cached_pack: stale after every optimizer step
            self._params[id(p)] = t
        return t

    def _clone(self, mod, memo):
        """A module of `mod`'s class with `mod`'s attributes (shared) and its own parameter / buffer / child tables."""
        if id(mod) in memo:
            return memo[id(mod)]
        new = copy.copy(mod)
        memo[id(mod)] = new
        d = new.__dict__
        d["_parameters"] = type(mod._parameters)((k, self._param(p)) for k, p in mod._parameters.items())
        d["_buffers"] = type(mod._buffers)((k, b if b is None else self._own.get(id(b), b)) for k, b in mod._buffers.items())
        d["_modules"] = type(mod._modules)((k, m if m is None else self._clone(m, memo)) for k, m in mod._modules.items())
        d["training"] = False
        d.pop("_ruled", None)                          # (the ViT's per-instance record of parameter ids)
        return new

    def arena_params(self):
        """[(arena slot, the teacher's parameter)] of every tensor that views optimizer.ema."""
        return sorted(((self._slot[k], t) for k, t in self._params.items()), key=lambda x: x[0])

    # ---- buffers -----------------------------------------------------------------------------------------------------
    def _segment_tables(self):
        src = [getattr(m, name) for m, name, _ in self._pairs]
        ptrs = [s.data_ptr() for s in src]
        if self._tables is None or ptrs != self._src_ptrs:     # (the student's buffers were replaced: .to(), a new tensor)
            self._tables = ops.ema_segment_tables([t for _, _, t in self._pairs], src)
            self._src_ptrs = ptrs
        return self._tables

    def update_buffers(self, d):
        """running_mean / running_var: buf_t = d * buf_t + (1 - d) * buf_s in one launch (d = 0 with buffers='copy');
        num_batches_tracked: copied.  Call it after optimizer.step() with optimizer.ema_decay_at(optimizer.step_count); the
        training steps do."""
        if not self._pairs:
            return
        ops.ema_segments(*self._segment_tables(), 0.0 if self.buffers == "copy" else float(d))
        self._copy_nbt()

    def _copy_nbt(self):
        # int64 counters: copied as pairs of fp32 words with the fp32 copy kernel (train._cat2 does the same for label maps)
        ops.eltwise(4, self._nbt_s.view(torch.float32).view(-1), None, out=self._nbt_t.view(torch.float32).view(-1))

    def _copy_buffers(self):
        if self._pairs:
            ops.ema_segments(*self._segment_tables(), 0.0)
            self._copy_nbt()

    def reset(self):
        """The teacher becomes the student: p -> ema and the BatchNorm buffers across.  For use after
        GradAllReducer.broadcast_params or after loading a student checkpoint."""
        opt = self.optimizer
        ops.eltwise(4, opt.p, None, out=opt.ema)
        self._copy_buffers()
        ops.weights_changed()
