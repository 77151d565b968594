"""Plain float64 restatement of the mean teacher's arithmetic (semivl_amd/optim.py: ema_from_cfg, ArenaOptimizer.ema_decay_at;
semivl_amd/ema.py; include/semivl_hip.h: svl_ema_segments_f32 and the `ema` argument of svl_adamw_step / svl_sgd_step), written
from their words, none of it from the kernels:

  schedule      d_t = decay, or with warm-up min(decay, 1 - 1 / t), t counted from 1, in double
  parameters    ema_t = d_t ema_{t-1} + (1 - d_t) p_t          (p_t: the weights AFTER step t's update)
  buffers       buf_t = d_t buf_{t-1} + (1 - d_t) s_t          (s_t: the student's running statistic after step t)

and the a-priori bound of one fp32 evaluation of  d * a + (1 - d) * b  as the kernels write it.  The kernels are handed d as
an fp32 number d32 and use omd32 = fp32(1 - d32) (svl_sgd_step and svl_ema_segments_f32 form it on the host from the double
difference; svl_adamw_step subtracts in fp32, which rounds the same exact difference the same way).  Given these two factors
the step kernels' chain has N_ROUNDINGS = 3 fp32 roundings as written (two products, one sum), two when the compiler
contracts a product and the sum into an FMA; svl_ema_segments_f32 pins its chain to N_ROUNDINGS_SEGMENTS = 2 (one rounded
product, one fused multiply-add).  With n roundings |fp32 result - exact| <= gamma(n) (|d32 a| + |omd32 b|),
gamma(n) = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1 applied to a
two-term inner product)."""
import numpy as np

U = 2.0 ** -24
N_ROUNDINGS = 3
N_ROUNDINGS_SEGMENTS = 2


def gamma(n):
    return n * U / (1.0 - n * U)


def f32(x):
    return float(np.float32(x))


def schedule(decay, warmup, t):
    """d_t in double; t = 1, 2, ..."""
    assert t >= 1
    return min(decay, 1.0 - 1.0 / t) if warmup else decay


def kernel_factors(d):
    """(d32, omd32): the two fp32 factors a kernel multiplies with when it is handed the double d."""
    d32 = f32(d)
    return d32, f32(1.0 - d32)


def step_ref(dst, src, d, n=N_ROUNDINGS):
    """One update as the kernels evaluate it, in float64 on float64 copies of the fp32 operands: (value, bound for a chain
    of n fp32 roundings)."""
    dst, src = np.asarray(dst, np.float64), np.asarray(src, np.float64)
    d32, omd32 = kernel_factors(d)
    a, b = d32 * dst, omd32 * src
    return a + b, gamma(n) * (np.abs(a) + np.abs(b))


def recursion(values, decay, warmup, start):
    """The exact recursion (double factors d_t, 1 - d_t) from `start` over values[0], values[1], ...: the list of ema_t."""
    e, out = np.asarray(start, np.float64), []
    for t, v in enumerate(values, 1):
        d = schedule(decay, warmup, t)
        e = d * e + (1.0 - d) * np.asarray(v, np.float64)
        out.append(e)
    return out


def geometric_sum(values, decay, start):
    """Closed form of the constant-decay recursion after T = len(values) steps:
    decay^T start + (1 - decay) sum_k decay^(T - k) v_k."""
    T = len(values)
    out = decay ** T * np.asarray(start, np.float64)
    for k, v in enumerate(values, 1):
        out = out + (1.0 - decay) * decay ** (T - k) * np.asarray(v, np.float64)
    return out


def compounded_bound(values, decay, warmup, start):
    """Bound of the fp32 chain's distance from the EXACT recursion after len(values) steps.  Per step the distance grows to
    d_t B_{t-1} (what was there, scaled) + gamma(3) (|d e| + |(1 - d) v|) (this step's roundings) + u (d |e| + |v|) (the two
    factors: d32 is d rounded, relative error <= u; omd32 = fp32(1 - d32) is off by at most u d from d32 and u (1 - d) from
    its own rounding, <= u in all).  |e|, |v| are taken from the exact recursion plus the bound so far."""
    e = np.asarray(start, np.float64)
    B = np.zeros_like(e)
    for t, v in enumerate(values, 1):
        v = np.asarray(v, np.float64)
        d = schedule(decay, warmup, t)
        mag_e = np.abs(e) + B
        B = d * B + gamma(N_ROUNDINGS) * (d * mag_e + (1.0 - d) * np.abs(v)) * (1.0 + U) + U * (d * mag_e + np.abs(v))
        e = d * e + (1.0 - d) * v
    return B
