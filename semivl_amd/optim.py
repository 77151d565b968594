"""The fused optimizers: ONE flat fp32 arena per optimizer (ArenaOptimizer), one kernel launch per step.

  semivl.py:123-125,339-345    mmcv param-wise AdamW + poly LR          -> FusedAdamW
  semivl.py:118-121,330-337    two-group SGD when cfg has no optimizer  -> FusedSGD.original
  mmseg build_optimizer        cfg['optimizer'] type AdamW / SGD        -> build_optimizer, optimizer_from_cfg
  mmcv OptimizerHook           optimizer_config = dict(grad_clip=...)   -> grad_clip_from_cfg, ArenaOptimizer.set_grad_clip
                               (not in semivl.py, which never clips)
  third_party/unimatch/eval.py:29,132-133  `--ema` reads checkpoint['ema_model'] -> ema_from_cfg, ArenaOptimizer.ema /
                               ema_decay_at: the average the mean teacher (ema.py) is built on
"""
import math
import numbers

import torch

from . import ops


def mmcv_param_groups(named_params, lr, weight_decay, custom_keys):
    """mmcv 1.4.4 DefaultOptimizerConstructor semantics (recalled): one group per parameter; custom keys
    sorted alphabetically then longest-first; the FIRST key contained in the parameter name sets lr_mult/decay_mult."""
    keys = sorted(sorted(custom_keys.keys()), key=len, reverse=True)
    out = []
    for name, p in named_params:
        g = dict(name=name, param=p, lr=lr, weight_decay=weight_decay)
        for k in keys:
            if k in name:
                g["lr"] = lr * custom_keys[k].get("lr_mult", 1.0)
                g["weight_decay"] = weight_decay * custom_keys[k].get("decay_mult", 1.0)
                break
        out.append(g)
    return out


def _trainable(name, prm):
    """The arena rule of every optimizer here: tensors that can receive a gradient.  `clip_encoder.*` (registered with
    requires_grad=True in the reference, never given a grad -- SURVEY App. E.2), `prompt_norm.*` of a ViT with prompt tokens
    (never called by the reference's forward: no grad either) and frozen backbone tensors are left untouched, which is also
    what torch's optimizers do for params whose .grad is None: no update, no weight decay."""
    return prm.requires_grad and not name.startswith("clip_encoder.") and ".prompt_norm." not in "." + name


def arena_layout(sizes):
    """(offsets, total) of segments of `sizes` floats, each padded to 4 floats: 16-byte aligned, so a float4 of the SGD
    kernel never straddles two segments.  No sizes: ([], 0)."""
    offs, o = [], 0
    for s in sizes:
        offs.append(o)
        o += (s + 3) // 4 * 4
    return offs, o


def _real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _check_grad_clip(max_norm, norm_type):
    """(max_norm as a float, norm_type as 2.0 or inf); ValueError for a max_norm that is no real number > 0,
    NotImplementedError for a norm_type other than 2 / 2.0 / float('inf') / 'inf'."""
    if not _real(max_norm) or not float(max_norm) > 0:
        raise ValueError("grad_clip: max_norm must be a real number > 0 (inf allowed), got %r" % (max_norm,))
    if norm_type == "inf":
        norm_type = math.inf
    if not _real(norm_type) or float(norm_type) not in (2.0, math.inf):
        raise NotImplementedError("grad_clip: norm_type %r is not supported: the arena's norm kernel forms the L2 norm (2) "
                                  "and the max norm (inf, 'inf')" % (norm_type,))
    return float(max_norm), float(norm_type)


def grad_clip_from_cfg(cfg):
    """mmcv's `optimizer_config = dict(grad_clip=dict(max_norm=..., norm_type=2))` (OptimizerHook, which calls
    torch.nn.utils.clip_grad_norm_(params, **grad_clip)) -> dict(max_norm, norm_type) for ArenaOptimizer, or None: no
    'optimizer_config' key, optimizer_config None, or grad_clip None.  norm_type: 2 / 2.0 / float('inf') / 'inf' (default 2).
    ValueError for values clip_grad_norm_ has no meaning for; NotImplementedError, naming the offender, for what torch / mmcv
    would do and this package does not: another norm_type, error_if_nonfinite=True (it needs the norm on the host: a sync
    every step), and any key of optimizer_config besides 'grad_clip' and 'type' (cumulative_iters, loss_scale, ... must not
    be ignored silently).  error_if_nonfinite=False and `foreach` are accepted: neither changes the result."""
    oc = cfg.get("optimizer_config")
    if oc is None:
        return None
    if not isinstance(oc, dict):
        raise ValueError("optimizer_config must be a dict or None, got %r" % (oc,))
    other = sorted(k for k in oc if k not in ("grad_clip", "type"))
    if other:
        raise NotImplementedError("optimizer_config keys %s are not supported (grad_clip only)" % other)
    gc = oc.get("grad_clip")
    if gc is None:
        return None
    if not isinstance(gc, dict):
        raise ValueError("optimizer_config['grad_clip'] must be a dict or None, got %r" % (gc,))
    stray = sorted(k for k in gc if k not in ("max_norm", "norm_type", "error_if_nonfinite", "foreach"))
    if stray:
        raise ValueError("grad_clip: unknown keys %s (clip_grad_norm_ takes max_norm, norm_type, error_if_nonfinite, "
                         "foreach)" % stray)
    if "max_norm" not in gc:
        raise ValueError("grad_clip needs max_norm")
    if gc.get("error_if_nonfinite", False):
        raise NotImplementedError("grad_clip: error_if_nonfinite=True is not supported: it needs the norm on the host, a "
                                  "sync every step (optimizer.grad_stats[3] is the flag, on the device)")
    max_norm, norm_type = _check_grad_clip(gc["max_norm"], gc.get("norm_type", 2))
    return dict(max_norm=max_norm, norm_type=norm_type)


def ema_from_cfg(cfg):
    """cfg['ema'] = dict(decay=0.996, warmup=True, teacher=True, buffers='ema') -> a dict with all four keys, or None
    without the key.  `decay` (required): a real number in [0, 1), no bool.  `warmup` (bool, default True): the decay of
    step t is min(decay, 1 - 1 / t) (ArenaOptimizer.ema_decay_at).  `teacher` (bool, default True): whether pseudo-labels
    come from the averaged weights or the average is only maintained.  `buffers`: 'ema' (default) or 'copy', the rule of
    the teacher's BatchNorm statistics (ema.EmaTeacher).  A non-dict, an unknown key or a value out of range raises
    ValueError naming it."""
    if "ema" not in cfg:
        return None
    e = cfg["ema"]
    if not isinstance(e, dict):
        raise ValueError("ema must be a dict(decay=..., warmup=True, teacher=True, buffers='ema'), got %r" % (e,))
    stray = sorted(k for k in e if k not in ("decay", "warmup", "teacher", "buffers"))
    if stray:
        raise ValueError("ema: unknown keys %s (decay, warmup, teacher, buffers)" % stray)
    if "decay" not in e:
        raise ValueError("ema needs decay")
    decay = e["decay"]
    if not _real(decay) or not 0.0 <= float(decay) < 1.0:
        raise ValueError("ema: decay must be a real number in [0, 1), got %r" % (decay,))
    out = dict(decay=float(decay))
    for k in ("warmup", "teacher"):
        v = e.get(k, True)
        if not isinstance(v, bool):
            raise ValueError("ema: %s must be a bool, got %r" % (k, v))
        out[k] = v
    out["buffers"] = e.get("buffers", "ema")
    if out["buffers"] not in ("ema", "copy"):
        raise ValueError("ema: buffers must be 'ema' or 'copy', got %r" % (out["buffers"],))
    return out


def ema_decay_schedule(decay, warmup, t):
    """The EMA decay of step t (1-based), in double: `decay`, or with warm-up min(decay, 1 - 1 / t) -- 0 at step 1 (the
    average starts as the first updated weights) and, while 1 - 1 / t < decay, the plain arithmetic mean of p_1 .. p_t."""
    if t < 1:
        raise ValueError("ema_decay_at: step %r (steps count from 1)" % (t,))
    return min(decay, 1.0 - 1.0 / t) if warmup else decay


class ArenaOptimizer:
    """ONE flat fp32 arena: parameters `p`, gradients `g` (`main_grad` views the model's backward writes into), the
    subclass's state buffers and optionally the EMA teacher, all laid out by arena_layout over `groups` (one dict per
    arena tensor: name, param, lr, weight_decay).  GradAllReducer and semivl_train_step rely on these attributes.

    A subclass validates its hyper-parameters, calls __init__ with its groups and the names of its state buffers, and
    supplies `_launch(gscale_dev)` (the step's one kernel; gscale_dev None: the host float grad_scale), `_hyper()` (the hyper-parameters every param group of state_dict()
    carries), `_state_entry(ai)` (state_dict()'s entry of arena tensor ai, or None) and `_load_state(sd, index)` (copies
    the entries in, returns the step count).

    `grad_clip` (None, or dict(max_norm, norm_type=2.0); set_grad_clip): torch.nn.utils.clip_grad_norm_ over all tensors of
    the arena before every step, as mmcv's OptimizerHook(grad_clip=...) does -- formed and applied on the device.  The norm
    is that of grad_scale * g (under GradAllReducer: of the averaged gradient, after the all-reduce, the same on every
    rank); `grad_stats` (fp32 [4] on the device, None without clipping) = {norm, coef, grad_scale * coef, non-finite flag}
    of the last step is what a training loop logs from.  g is not rewritten: the step kernel reads grad_stats[2] as its
    gradient scale.  Non-finite gradients: as in torch with error_if_nonfinite=False, nothing is skipped.  Configuration,
    not state: state_dict() does not carry it."""

    def __init__(self, model, groups, lr, wd, ema_decay, state, grad_clip=None):
        self.lr, self.wd, self.groups = lr, wd, groups
        arena_index = {id(g_["param"]): i for i, g_ in enumerate(groups)}
        self.all_params = [(n, arena_index.get(id(p))) for n, p in model.named_parameters()]   # (name, arena slot | None)
        sizes = [g_["param"].numel() for g_ in groups]
        self._offs, self.total = arena_layout(sizes)
        dev = groups[0]["param"].device
        self.p = ops.zeros(self.total, device=dev)
        self.g = ops.zeros(self.total, device=dev)
        for name in state:
            setattr(self, name, ops.zeros(self.total, device=dev))
        for g_, off, s in zip(groups, self._offs, sizes):
            prm = g_["param"]
            view = self.p[off:off + s].view(prm.shape)
            ops.eltwise(4, prm.data.contiguous().view(-1), None, out=view.view(-1))
            prm.data = view
            prm.main_grad = self.g[off:off + s].view(prm.shape)
            g_["initial_lr"] = g_["lr"]
        self.ema = self.p.clone() if ema_decay is not None else None
        self.ema_decay = ema_decay or 0.0
        self.ema_warmup = False   # (set_ema_warmup / cfg['ema']: the decay of step t is min(ema_decay, 1 - 1 / t))
        self.seg_off = torch.tensor(self._offs + [self.total], dtype=torch.int64, device=dev)
        self.seg_wd = torch.tensor([g_["weight_decay"] for g_ in groups], dtype=torch.float32, device=dev)
        self._lr_host = torch.tensor([g_["lr"] for g_ in groups], dtype=torch.float32)
        if torch.cuda.is_available():
            self._lr_host = self._lr_host.pin_memory()
        self.seg_lr = self._lr_host.to(dev)
        self._lr_evt = None
        self.step_count = 0
        self.grad_scale = 1.0
        self._lr_factor = 1.0     # the schedule's current factor (poly_lr): lr of the groups outside the arena
        self.grad_clip, self.grad_stats, self._clip_ws = None, None, None
        if grad_clip is not None:
            self.set_grad_clip(**grad_clip)

    def set_grad_clip(self, max_norm, norm_type=2.0):
        """Clip the arena's gradient norm to max_norm before every step (max_norm=inf: only report it); None: off."""
        if max_norm is None:
            self.grad_clip, self.grad_stats = None, None
            return
        max_norm, norm_type = _check_grad_clip(max_norm, norm_type)
        self.grad_clip = dict(max_norm=max_norm, norm_type=norm_type)
        if self.grad_stats is None:
            self.grad_stats = ops.zeros(4, device=self.g.device)
        if self._clip_ws is None:
            self._clip_ws = ops.grad_clip_ws(self.g)

    def set_ema_warmup(self, warmup=True):
        """Warm the EMA up (cfg['ema']['warmup']): see ema_decay_at.  Configuration, not state, like grad_clip."""
        if not isinstance(warmup, bool):
            raise ValueError("ema: warmup must be a bool, got %r" % (warmup,))
        if warmup and self.ema is None:
            raise ValueError("ema: warmup without an EMA arena (build the optimizer with ema_decay= or cfg['ema'])")
        self.ema_warmup = warmup

    def ema_decay_at(self, t):
        """d_t, the EMA decay the step kernel is handed at step t (1-based: step_count after its increment), formed on the
        host in double: ema_decay, or with warm-up min(ema_decay, 1 - 1 / t)."""
        return ema_decay_schedule(self.ema_decay, self.ema_warmup, t)

    @property
    def param_groups(self):
        return self.groups

    def zero_grad(self):
        ops.fill(self.g, 0.0)

    def _fold_autograd_grads(self):
        """Gradients that reached a parameter through torch autograd instead of the main_grad sink (e.g. pos_embed
        behind its bicubic resize at 801x801) are added to the arena."""
        for g_ in self.groups:
            prm = g_["param"]
            if prm.grad is not None:
                ops.add(prm.main_grad.view(-1), prm.grad.contiguous().view(-1), out=prm.main_grad.view(-1))
                prm.grad = None

    def step(self):
        self._fold_autograd_grads()
        self.step_count += 1
        if self.grad_clip is None:
            self._launch(None)
        else:
            ops.grad_clip(self.g, self.grad_clip["max_norm"], self.grad_clip["norm_type"], gscale=self.grad_scale,
                          stats=self.grad_stats, ws=self._clip_ws)
            self._launch(self.grad_stats[2:3])
        ops.weights_changed()    # cached bf16 planes of the trainable weights are stale now (ops.weight_planes)

    def _seg(self, buf, ai):
        """Arena tensor ai's part of `buf`, in the parameter's shape."""
        off, prm = self._offs[ai], self.groups[ai]["param"]
        return buf[off:off + prm.numel()].view(prm.shape)

    def _stage_lr(self, lrs):
        """New per-segment learning rates (Python floats; fp32 only here) through the pinned staging buffer."""
        # the buffer may still be the source of the previous call's queued copy: wait for THAT copy (issued a whole step
        # ago in the training loop, so this never stalls there) before overwriting it
        if self._lr_evt is not None:
            self._lr_evt.synchronize()
        for i, lr in enumerate(lrs):
            self._lr_host[i] = lr
        self.seg_lr.copy_(self._lr_host, non_blocking=True)
        if self.seg_lr.is_cuda:
            self._lr_evt = torch.cuda.Event()
            self._lr_evt.record()

    def poly_lr(self, iters, max_iters, power=0.9, warmup_iters=0, warmup_ratio=1e-6):
        """semivl.py:339-345: applied after the step, for the next one; linear warm-up while iters < warmup_iters
        (semivl.py:339-342: lr = initial_lr * (1 - (1 - iters / warmup_iters) * (1 - warmup_ratio)))."""
        if iters < warmup_iters:
            f = 1 - (1 - iters / warmup_iters) * (1 - warmup_ratio)
        else:
            f = (1 - iters / max_iters) ** power
        self._lr_factor = f
        for g_ in self.groups:
            g_["lr"] = g_["initial_lr"] * f
        self._stage_lr([g_["lr"] for g_ in self.groups])

    def state_dict(self):
        """The layout of the reference's checkpoint entry (`semivl.py:428` stores `optimizer.state_dict()` of a torch
        optimizer built by mmcv's DefaultOptimizerConstructor): ONE param group per tensor of `model.named_parameters()`,
        in that order, frozen tensors and `clip_encoder.*` included (mmcv lists them with the base lr / weight decay; they
        never receive a gradient, so they have no `state` entry); state[i] = the subclass's entry for the tensors of the
        arena.  Index-compatible with the reference in both directions
        (tests/test_model_gpu.py::test_optimizer_state_dict_is_index_compatible).  `names` (all parameters, same order) is
        stored in addition and verified on load."""
        state, groups = {}, []
        for j, (name, ai) in enumerate(self.all_params):
            if ai is None:      # mmcv lists them with the base lr; semivl.py:124-125 gives EVERY group an initial_lr and
                # :341-345 re-schedules every group from it, so a reference-style loop can load this dict as it is
                groups.append(dict(lr=self.lr * self._lr_factor, initial_lr=self.lr, weight_decay=self.wd,
                                   **self._hyper(), params=[j]))
                continue
            g_ = self.groups[ai]
            entry = self._state_entry(ai)
            if entry is not None:
                state[j] = entry
            groups.append(dict(lr=g_["lr"], initial_lr=g_["initial_lr"], weight_decay=g_["weight_decay"],
                               **self._hyper(), params=[j]))
        return dict(state=state, param_groups=groups, names=[n for n, _ in self.all_params])

    def load_state_dict(self, sd):
        """Accepts what state_dict() returns and what the torch optimizer, built by mmcv's constructor, returns."""
        pg = sd["param_groups"]
        assert len(pg) == len(self.all_params), "optimizer state does not match this model"
        self._load_tensor_groups(sd, [(j, ai) for j, (_, ai) in enumerate(self.all_params) if ai is not None],
                                 [n for n, _ in self.all_params])
        for j, (_, ai) in enumerate(self.all_params):
            if ai is None and pg[j].get("initial_lr"):
                self._lr_factor = pg[j]["lr"] / pg[j]["initial_lr"]
                break

    def _load_tensor_groups(self, sd, index, names):
        """One param group per tensor: index = [(number in sd, arena slot)], names = sd's parameter names in its order."""
        for j, ai in index:
            g_, sg = self.groups[ai], sd["param_groups"][j]
            assert [int(k) for k in sg["params"]] == [j], "one parameter per group expected (mmcv constructor layout)"
            g_["lr"], g_["initial_lr"] = sg["lr"], sg.get("initial_lr", g_["initial_lr"])
        self._finish_load(sd, index, names)

    def _finish_load(self, sd, index, names):
        """What every layout shares once the groups' lr is set: the checks, the state entries, the step count, seg_lr."""
        if "names" in sd:
            assert list(sd["names"]) == names, "optimizer state was saved for different parameters: %s" % (
                sorted(set(sd["names"]) ^ set(names))[:6],)
        stray = set(sd["state"]) - {j for j, _ in index}
        assert not stray, "state for parameters this model never trains: %s" % sorted(stray)[:6]
        self.step_count = self._load_state(sd, index)
        self._stage_lr([g_["lr"] for g_ in self.groups])


class FusedAdamW(ArenaOptimizer):
    """torch.optim.AdamW semantics over the arena: parameters, gradients, exp_avg `m`, exp_avg_sq `v`; one svl_adamw_step
    launch per step (28 B/param of HBM traffic)."""

    def __init__(self, model, optimizer_cfg, ema_decay=None, grad_clip=None):
        assert optimizer_cfg.get("type", "AdamW") == "AdamW"
        lr, wd = optimizer_cfg["lr"], optimizer_cfg.get("weight_decay", 0.01)
        self.betas, self.eps = optimizer_cfg.get("betas", (0.9, 0.999)), optimizer_cfg.get("eps", 1e-8)
        ck = optimizer_cfg.get("paramwise_cfg", {}).get("custom_keys", {})
        named = [(n, p) for n, p in model.named_parameters() if _trainable(n, p)]
        super().__init__(model, mmcv_param_groups(named, lr, wd, ck), lr, wd, ema_decay, ("m", "v"), grad_clip)

    def _launch(self, gscale_dev):
        ops.adamw_step(self.p, self.g, self.m, self.v, self.seg_off, self.seg_lr, self.seg_wd, len(self.groups),
                       self.betas[0], self.betas[1], self.eps, self.step_count, self.grad_scale, self.ema,
                       self.ema_decay_at(self.step_count), gscale_dev=gscale_dev)

    def _hyper(self):
        return dict(betas=tuple(self.betas), eps=self.eps, amsgrad=False)

    def _state_entry(self, ai):
        if self.step_count > 0:
            return dict(step=torch.tensor(float(self.step_count)),
                        exp_avg=self._seg(self.m, ai).detach().cpu().clone(),
                        exp_avg_sq=self._seg(self.v, ai).detach().cpu().clone())

    def load_state_dict(self, sd):
        """Accepts the reference layout (one group per model parameter) and the compact round-1/2 layout of this package
        (one group per arena tensor)."""
        if len(sd["param_groups"]) == len(self.all_params):
            return super().load_state_dict(sd)
        assert len(sd["param_groups"]) == len(self.groups), "optimizer state does not match this model"
        self._load_tensor_groups(sd, [(i, i) for i in range(len(self.groups))], [g_.get("name", "") for g_ in self.groups])

    def _load_state(self, sd, index):
        steps = set()
        for j, ai in index:
            st = sd["state"].get(j)
            if st is not None:
                shape = tuple(self.groups[ai]["param"].shape)
                assert tuple(st["exp_avg"].shape) == shape, (self.groups[ai].get("name"), st["exp_avg"].shape)
                self._seg(self.m, ai).copy_(st["exp_avg"])
                self._seg(self.v, ai).copy_(st["exp_avg_sq"].reshape(shape))
                steps.add(int(st["step"]))
        assert len(steps) <= 1, "per-tensor step counts differ"
        return steps.pop() if steps else 0


def sgd_original_groups(model, lr, lr_multi, weight_decay=1e-4):
    """The two param groups of semivl.py:118-121, in the reference's order, as lists of (name, param): group 0 =
    model.backbone.parameters() (frozen ones included), group 1 = every named parameter whose name lacks 'backbone'
    (clip_encoder.* falls here).  torch numbers the parameters of a state_dict through the groups in this order.  Returns
    (members, index, groups): members[k] = [(name, param)], index[name] = torch's parameter index, groups = one dict per
    ARENA tensor (name, param, lr, weight_decay, group) in model.named_parameters() order, like mmcv_param_groups'."""
    named = list(model.named_parameters())
    members = [[("backbone." + n, p) for n, p in model.backbone.named_parameters()],
               [(n, p) for n, p in named if "backbone" not in n]]
    which, index = {}, {}
    for k, mem in enumerate(members):
        for n, p in mem:
            if id(p) in which:
                raise ValueError("parameter %s appears in more than one SGD param group" % n)   # torch raises too
            which[id(p)] = k
            index[n] = len(index)
    stray = [n for n, p in named if id(p) not in which]
    if stray:
        raise ValueError("parameters in neither group of the reference's SGD recipe (name contains 'backbone' but not under "
                         "model.backbone): %s" % stray[:6])
    lrs = (lr, lr * lr_multi)
    groups = [dict(name=n, param=p, lr=lrs[which[id(p)]], weight_decay=weight_decay, group=which[id(p)])
              for n, p in named if _trainable(n, p)]
    return members, index, groups


def sgd_original_lr(lr, lr_multi, iters, max_iters, warmup_iters=0, warmup_ratio=1e-6):
    """semivl.py:330-337 in its order of operations (Python floats): (lr of group 0, lr of group 1) for the next step."""
    if iters < warmup_iters:
        k = (1 - iters / warmup_iters) * (1 - warmup_ratio)
        cur = lr * (1 - k)
    else:
        cur = lr * (1 - iters / max_iters) ** 0.9
    return cur, cur * lr_multi


class FusedSGD(ArenaOptimizer):
    """torch.optim.SGD semantics over the arena (parameters, gradients, momentum buffer `m`, None without momentum): one
    svl_sgd_step launch per step, 20 B/param of HBM traffic (28 with the EMA teacher).

    FusedSGD(model, optimizer_cfg): cfg['optimizer'] = dict(type='SGD', lr, momentum, weight_decay, dampening, nesterov,
    paramwise_cfg) through mmcv's per-parameter groups.  FusedSGD.original(model, lr, lr_multi): the optimizer the
    reference builds when cfg has no 'optimizer' key (semivl.py:118-121), re-scheduled by semivl.py:330-337; its
    param_groups, state_dict() and poly_lr follow the reference's two groups (`lr_multi` set), everything else is shared."""

    def __init__(self, model, optimizer_cfg, ema_decay=None, *, lr_multi=None, grad_clip=None):
        if optimizer_cfg.get("type", "SGD") != "SGD":
            raise ValueError("FusedSGD got optimizer type %r" % (optimizer_cfg.get("type"),))
        momentum, dampening = optimizer_cfg.get("momentum", 0.0), optimizer_cfg.get("dampening", 0.0)
        nesterov = bool(optimizer_cfg.get("nesterov", False))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")      # torch.optim.SGD's refusal
        self.momentum, self.dampening, self.nesterov, self.lr_multi = momentum, dampening, nesterov, lr_multi
        lr, wd = optimizer_cfg["lr"], optimizer_cfg.get("weight_decay", 0.0)
        if lr_multi is None:
            ck = optimizer_cfg.get("paramwise_cfg", {}).get("custom_keys", {})
            named = [(n, p) for n, p in model.named_parameters() if _trainable(n, p)]
            self._members, self._index, groups = None, None, mmcv_param_groups(named, lr, wd, ck)
        else:
            self._members, self._index, groups = sgd_original_groups(model, lr, lr_multi, wd)
            self._pg = [dict(lr=lr), dict(lr=lr * lr_multi)]
        self.m = None
        super().__init__(model, groups, lr, wd, ema_decay, ("m",) if momentum != 0 else (), grad_clip)

    @classmethod
    def original(cls, model, lr, lr_multi, momentum=0.9, weight_decay=1e-4, ema_decay=None, grad_clip=None):
        return cls(model, dict(type="SGD", lr=lr, momentum=momentum, weight_decay=weight_decay), ema_decay,
                   lr_multi=lr_multi, grad_clip=grad_clip)

    @property
    def param_groups(self):
        """Per-tensor groups (mmcv layout), or the reference's two groups for the `original` recipe."""
        return self.groups if self._members is None else self._pg

    def _launch(self, gscale_dev):
        ops.sgd_step(self.p, self.g, self.m, self.seg_off, self.seg_lr, self.seg_wd, len(self.groups), self.momentum,
                     self.dampening, self.nesterov, self.step_count, self.grad_scale, self.ema,
                     self.ema_decay_at(self.step_count), gscale_dev=gscale_dev)

    def _hyper(self):
        return dict(momentum=self.momentum, dampening=self.dampening, nesterov=self.nesterov, maximize=False, foreach=None,
                    differentiable=False, fused=None)

    def _state_entry(self, ai):
        if self.step_count > 0 and self.m is not None:
            return dict(momentum_buffer=self._seg(self.m, ai).detach().cpu().clone())

    def _original_index(self):
        """`original`: (names in torch's numbering, [(number, arena slot)] of the arena's tensors)."""
        names, slot = sorted(self._index, key=self._index.get), dict(self.all_params)
        return names, [(j, slot[n]) for j, n in enumerate(names) if slot[n] is not None]

    def state_dict(self):
        """torch.optim.SGD's layout, as the reference saves it (semivl.py:428).  `original`: the two param groups of
        semivl.py:118-121 with `params` numbered through the groups in order; mmcv style: ArenaOptimizer.state_dict's
        layout.  state[i] = {'momentum_buffer'} for the tensors of the arena once a step has run.  `step_count` and
        `names` are stored in addition; torch ignores them, and a dict saved by torch loads without them."""
        if self._members is None:
            sd = super().state_dict()
        else:
            names, index = self._original_index()
            entries = [(j, self._state_entry(ai)) for j, ai in index]
            sd = dict(state={j: e for j, e in entries if e is not None},
                      param_groups=[dict(lr=self._pg[k]["lr"], weight_decay=self.wd, **self._hyper(),
                                         params=[self._index[n] for n, _ in mem]) for k, mem in enumerate(self._members)],
                      names=names)
        sd["step_count"] = self.step_count
        return sd

    def load_state_dict(self, sd):
        """Accepts what state_dict() returns and what torch.optim.SGD, built the same way, returns."""
        if self._members is None:
            return super().load_state_dict(sd)
        pg = sd["param_groups"]
        assert len(pg) == 2, "the reference's SGD recipe has two param groups"
        for k, mem in enumerate(self._members):
            assert [int(i) for i in pg[k]["params"]] == [self._index[n] for n, _ in mem], "param group %d differs" % k
            self._pg[k]["lr"] = pg[k]["lr"]
        for g_ in self.groups:
            g_["lr"] = pg[g_["group"]]["lr"]
        names, index = self._original_index()
        self._finish_load(sd, index, names)

    def _load_state(self, sd, index):
        loaded = 0
        for j, ai in index:
            st = sd["state"].get(j)
            if st is not None and st.get("momentum_buffer") is not None and self.m is not None:
                buf = self._seg(self.m, ai)
                assert tuple(st["momentum_buffer"].shape) == tuple(buf.shape), (self.groups[ai].get("name"),
                                                                               st["momentum_buffer"].shape)
                buf.copy_(st["momentum_buffer"])
                loaded += 1
        assert loaded in (0, len(index)), "momentum buffers for only some of the trained tensors"
        # torch's SGD keeps no step count: a momentum buffer exists <=> a step has run, which is all the update rule asks
        return int(sd.get("step_count", 1 if loaded else 0))

    def poly_lr(self, iters, max_iters, power=0.9, warmup_iters=0, warmup_ratio=1e-6):
        """Applied after the step, for the next one.  `original`: semivl.py:330-337 (lr = cfg lr * f, then lr * lr_multi for
        group 1, exponent 0.9); mmcv style: semivl.py:339-345, ArenaOptimizer.poly_lr.  Python floats throughout."""
        if self._members is None:
            return super().poly_lr(iters, max_iters, power, warmup_iters, warmup_ratio)
        lrs = sgd_original_lr(self.lr, self.lr_multi, iters, max_iters, warmup_iters, warmup_ratio)
        self._lr_factor = lrs[0] / self.lr if self.lr else 1.0
        for k in (0, 1):
            self._pg[k]["lr"] = lrs[k]
        for g_ in self.groups:
            g_["lr"] = lrs[g_["group"]]
        self._stage_lr([g_["lr"] for g_ in self.groups])


def build_optimizer(model, optimizer_cfg, ema_decay=None, grad_clip=None):
    """mmseg's build_optimizer for the types this package runs fused: AdamW (exp 40-44) and SGD.  `grad_clip`: None or
    dict(max_norm, norm_type) (ArenaOptimizer); passed on only when set."""
    kind = optimizer_cfg.get("type", "AdamW")
    clip = {} if grad_clip is None else dict(grad_clip=grad_clip)
    if kind == "AdamW":
        return FusedAdamW(model, optimizer_cfg, ema_decay=ema_decay, **clip)
    if kind == "SGD":
        return FusedSGD(model, optimizer_cfg, ema_decay=ema_decay, **clip)
    raise ValueError("optimizer type %r is not supported (AdamW, SGD)" % (kind,))


def optimizer_from_cfg(model, cfg, ema_decay=None):
    """semivl.py:118-125: without an 'optimizer' key the reference's two-group SGD (cfg['lr'], cfg['lr_multi']), with it
    whatever the key builds.  cfg['optimizer_config'] in mmcv's spelling (grad_clip_from_cfg) switches gradient-norm clipping
    on for either; without the key, or with grad_clip=None, the optimizer launches what it always did.
    cfg['ema'] (ema_from_cfg) builds either with the EMA arena: decay and warm-up from the key (`ema_cfg` on the optimizer
    keeps the whole dict for ema.EmaTeacher.from_cfg).  An explicit `ema_decay=` together with the key is a ValueError;
    `ema_decay=` alone is a constant decay without warm-up, as before."""
    grad_clip = grad_clip_from_cfg(cfg)
    ema = ema_from_cfg(cfg)
    if ema is not None and ema_decay is not None:
        raise ValueError("optimizer_from_cfg: ema_decay=%r and cfg['ema'] both set the EMA decay; give one" % (ema_decay,))
    if ema is not None:
        ema_decay = ema["decay"]
    clip = {} if grad_clip is None else dict(grad_clip=grad_clip)
    if "optimizer" not in cfg:
        opt = FusedSGD.original(model, cfg["lr"], cfg["lr_multi"], ema_decay=ema_decay, **clip)
    else:
        opt = build_optimizer(model, cfg["optimizer"], ema_decay=ema_decay, **clip)
    if ema is not None:
        opt.set_ema_warmup(ema["warmup"])
        opt.ema_cfg = ema
    return opt
