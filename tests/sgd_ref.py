"""Plain float64 restatement of svl_sgd_step (include/semivl_hip.h: torch.optim.SGD with maximize=False over a flat arena of
segments, each with its own learning rate and weight decay), written from the header's formula, not from the kernel, with
the a-priori fp32 error bound of the kernel's chain and the seeded cases tests/test_sgd_ref.py (CPU) and
tests/test_sgd_gpu.py share.  No tolerance is picked here or there (the convention of tests/spatial_ref.py).

Bound.  An fp32 evaluation of a sum of products in which every term passes through at most k roundings errs by at most
gamma(k) * sum |term|, gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).  A
fused multiply-add the compiler contracts only removes a rounding.  The kernel's expression tree, every fp32 rounding counted
(the arrays, lr, wd, momentum, gscale and ema_decay ARE fp32 numbers; 1 - dampening and 1 - ema_decay are formed in double
on the host and rounded to fp32 once):

    t1 = fl(g * gscale), t2 = fl(wd * p), d = fl(t1 + t2)                      terms g*gscale, wd*p: 2 roundings each
    step == 1:  m = d                                                          k_m = 2
    step >  1:  c = fl(1 - dampening); m = fl(fl(momentum * m) + fl(c * d))    d's terms 2 + 1 (c) + 1 + 1 = 5, m's 2: k_m = 5
    nesterov:   d' = fl(d + fl(momentum * m))                                  m's terms k_m + 2, d's own 3:  k_d = k_m + 2
    otherwise:  d' = m  (k_d = k_m),  or d' = d without momentum (k_d = 2)
    p' = fl(p - fl(lr * d'))                                                   k_p = k_d + 2; p's own term 1
    e = fl(1 - ema_decay); ema' = fl(fl(ema_decay * ema) + fl(e * p'))         k_ema = k_p + 3; ema's own term 2

so k_p is 4 without momentum, 4 / 7 with it (first / later steps) and 6 / 9 with nesterov."""
import numpy as np
import torch

from small_kernel_ref import GUARD, SENTINEL, U, guard_intact, guarded  # noqa: F401  (re-exported for the two test files)

AGUARD = 64          # guard elements that keep the payload 16-byte aligned (the kernel's float4 accesses need it)


def gamma(n):
    return n * U / (1.0 - n * U)


def f32(x):
    """The fp32 number a float argument of the C entry point carries, as a Python float."""
    return float(np.float32(x))


def chain_lengths(momentum, nesterov, step):
    """(k_m, k_p, k_ema) of the derivation above."""
    if momentum == 0:
        k_m, k_d = 0, 2
    else:
        k_m = 2 if step == 1 else 5
        k_d = k_m + 2 if nesterov else k_m
    return k_m, k_d + 2, k_d + 5


def sgd_ref(p, g, m, seg_off, seg_lr, seg_wd, nseg, total, momentum, dampening, nesterov, step, gscale=1.0, ema=None,
            ema_decay=0.0):
    """The kernel's arguments (flat fp32 arrays or tensors, segment tables; m / ema may be None) -> dict of float64 numpy
    arrays p, m, ema after the step and p_bound, m_bound, ema_bound, the a-priori bounds on an fp32 evaluation's error per
    element (None where the array is absent), plus k = (k_m, k_p, k_ema)."""
    a64 = lambda t: None if t is None else np.asarray(torch.as_tensor(t).detach().cpu().numpy(), dtype=np.float64)[:total]
    p, g, m, ema = a64(p), a64(g), a64(m), a64(ema)
    off = [int(v) for v in torch.as_tensor(seg_off).tolist()[:nseg]] + [int(total)]
    assert off[0] == 0 and all(b > a for a, b in zip(off, off[1:])), "segments must tile [0, total)"
    seg = np.repeat(np.arange(nseg), np.diff(off))
    lr = np.asarray(torch.as_tensor(seg_lr).cpu().numpy(), dtype=np.float64)[seg]
    wd = np.asarray(torch.as_tensor(seg_wd).cpu().numpy(), dtype=np.float64)[seg]
    mom, damp, gs, dec = f32(momentum), f32(dampening), f32(gscale), f32(ema_decay)
    if nesterov and (mom <= 0 or damp != 0):
        raise ValueError("nesterov needs a momentum and zero dampening")
    if mom != 0 and m is None:
        raise ValueError("momentum needs a buffer")
    k_m, k_p, k_ema = chain_lengths(mom, nesterov, step)
    d = g * gs + wd * p
    t_d = np.abs(g * gs) + np.abs(wd * p)                 # sums of |terms|, carried beside the values
    m_new = m_bound = None
    if mom != 0:
        if step == 1:
            m_new, t_m = d.copy(), t_d
        else:
            m_new = mom * m + (1.0 - damp) * d
            t_m = np.abs(mom * m) + abs(1.0 - damp) * t_d
        m_bound = gamma(k_m) * t_m
        if nesterov:
            d, t_d = d + mom * m_new, t_d + abs(mom) * t_m
        else:
            d, t_d = m_new, t_m
    p_new = p - lr * d
    t_p = np.abs(p) + np.abs(lr) * t_d
    out = dict(p=p_new, m=m_new, ema=None, p_bound=gamma(k_p) * t_p, m_bound=m_bound, ema_bound=None, k=(k_m, k_p, k_ema))
    if ema is not None:
        out["ema"] = dec * ema + (1.0 - dec) * p_new
        out["ema_bound"] = gamma(k_ema) * (np.abs(dec * ema) + abs(1.0 - dec) * t_p)
    return out


# ------------------------------------------------------------------------------------------------ shared cases
MOM, DAMP = f32(0.9), f32(0.3)
MODES = {            # every scalar is an fp32 number, so torch (Python floats) and the kernel (C floats) see the same values
    "momentum": dict(momentum=MOM, dampening=0.0, nesterov=False, gscale=1.0),
    "dampening": dict(momentum=MOM, dampening=DAMP, nesterov=False, gscale=1.0),
    "nesterov": dict(momentum=MOM, dampening=0.0, nesterov=True, gscale=1.0),
    "no_momentum": dict(momentum=0.0, dampening=0.0, nesterov=False, gscale=1.0),
    "gscale": dict(momentum=MOM, dampening=0.0, nesterov=False, gscale=0.5),
    "gscale_odd": dict(momentum=MOM, dampening=DAMP, nesterov=False, gscale=f32(1.0 / 3.0)),
}
SIZES = {
    "ragged": [1, 3, 4, 5, 7, 64, 1023],                          # padding, a segment under one float4, a boundary inside a wave
    "one": [777],                                                 # nseg = 1
    "many": [4 + (i * 7) % 9 for i in range(300)],                # 300 segments of 4..12 floats: many inside one block
    "small": [5, 30],                                             # total smaller than one block
}


def arena(sizes, seed, steps=3):
    """A FusedSGD-style arena: segments padded to 4 floats (padding lanes zero in p and every g), per-segment lr and weight
    decay (some zero), `steps` gradients.  Returns dict(p, gs, seg_off, seg_lr, seg_wd, nseg, total, pad) of CPU tensors."""
    gen = torch.Generator().manual_seed(seed)
    offs, o = [], 0
    for s in sizes:
        offs.append(o)
        o += (s + 3) // 4 * 4
    total, nseg = o, len(sizes)
    live = torch.zeros(total, dtype=torch.bool)
    for a, s in zip(offs, sizes):
        live[a:a + s] = True
    p = torch.randn(total, generator=gen) * live
    gs = [torch.randn(total, generator=gen) * 0.1 * live for _ in range(steps)]
    seg_lr = (10.0 ** (-1 - 3 * torch.rand(nseg, generator=gen))).float()
    seg_wd = torch.where(torch.arange(nseg) % 3 == 1, torch.zeros(nseg), 10.0 ** (-2 - 2 * torch.rand(nseg, generator=gen))).float()
    return dict(p=p, gs=gs, seg_off=torch.tensor(offs + [total], dtype=torch.int64), seg_lr=seg_lr, seg_wd=seg_wd,
                nseg=nseg, total=total, pad=~live, sizes=list(sizes), offs=offs)


def torch_sgd(case, mode, dtype):
    """torch.optim.SGD over one tensor per segment (its own lr / weight decay), on the case's values in `dtype`.  Returns
    (optimizer, params); the caller sets .grad (already multiplied by gscale) and steps."""
    prm = [case["p"][a:a + s].to(dtype).clone().requires_grad_(True) for a, s in zip(case["offs"], case["sizes"])]
    opt = torch.optim.SGD([dict(params=[q], lr=float(case["seg_lr"][i]), weight_decay=float(case["seg_wd"][i]))
                           for i, q in enumerate(prm)], lr=1.0, momentum=mode["momentum"], dampening=mode["dampening"],
                          nesterov=mode["nesterov"])
    return opt, prm


def flat(case, tensors, dtype=torch.float64):
    """Per-segment tensors -> the padded flat arena layout (padding zero)."""
    out = torch.zeros(case["total"], dtype=dtype)
    for a, s, t in zip(case["offs"], case["sizes"], tensors):
        out[a:a + s] = t.detach().to(dtype)
    return out
