"""svl_gemm_desc restated in float64 (plain torch on the CPU), written from the words of include/semivl_hip.h.

`reference(desc, tensors) -> (C64, written_mask, bound)` evaluates one descriptor by explicit index arithmetic: every logical
operand element A[z](m, k) / B[z](n, k) is gathered from the flat source buffers at the address the header gives for its
operand mode, the contraction and the epilogue run in float64, and the result is scattered into a float64 copy of the output
buffer together with a boolean mask of the elements the descriptor addresses.  Nothing here knows about tiles, loaders or
dispatch: the kernels are compared WITH this file (tests/test_gemm_desc_gpu.py), and this file is compared with independent
torch operations (tests/test_gemm_desc_ref.py).

The descriptor is a plain dict (see `desc()` for the keys and their defaults); tensors are named, flat buffers:
`tensors[name]` is any 1-D tensor, operands refer to it by name plus an element offset.

The bound
---------
fp32 families compute every output element as a k-ordered chain of fp32 fused multiply-adds followed by a few fp32 epilogue
operations.  With u = 2^-24 and K' the length of the chain (the slab length under split-K), the standard forward error
analysis (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1) gives, for ANY order of the K' terms,

    |fl(sum_k a_k b_k) - sum_k a_k b_k| <= gamma_K' * sum_k |a_k| |b_k|,        gamma_n = n u / (1 - n u).

The epilogue adds at most five more roundings to a value that is a sum of the terms alpha * acc, bias, resid and C_in:
(1) alpha * acc, (2) + bias, (3) the multiply of SVL_ACT_MUL_DGELU, (4) + resid, (5) + C_in.  Each rounding is relative to a
partial sum that is bounded by the sum of the terms' magnitudes, so the whole result obeys

    |C - C64| <= gamma_(K' + 5) * (|alpha| |A|.|B| + |bias| + |resid| + |C_in|).

gamma_(K'+5) <= (K' + c) u with c = 6 while (K' + 5)(K' + 6) u <= 1, i.e. K' <= 4089 (c = 5 roundings + 1 for the
second-order term); the code evaluates gamma_(K'+5) itself, so longer chains are covered as well.  ReLU and the
SVL_ACT_MUL_DRELU select are 1-Lipschitz and exact.  Through GELU the error of the argument is multiplied by the function's
Lipschitz constant GELU_LIPSCHITZ = max |GELU'| = 1.12890...  (attained at x = +sqrt(2): GELU'(x) = Phi(x) + x phi(x)), and
the distance of an fp32 erf-GELU from the float64 one is added.  That last term cannot be derived; it is MEASURED as the
distance of torch's own fp32 CPU F.gelu from the float64 function on the same fp32 arguments (4 000 001 points over [-12, 12]
plus all powers of two down to 2^-40), relative to |x|, and given a factor 2 (two implementations of erff):

    ERF_GELU_REL  = 2 x 3.53e-7 -> 7.1e-7        |gelu32(x) - gelu64(x)| <= ERF_GELU_REL * |x|
    ERF_DGELU_ABS = 2 x 2.74e-7 -> 5.5e-7        |gelu'32(z) - gelu'64(z)| <= ERF_DGELU_ABS      (|gelu'| <= 1.13)

(tests/test_gemm_desc_ref.py::test_erf_terms_are_twice_the_measured_distance re-measures both.)  The B producers evaluate
their operand in fp32 before the chain: SVL_B_NC_GELU elements carry the ERF_GELU_REL term; SVL_B_NC_LN elements
(x - mean) * rstd * gamma + beta carry four roundings, gamma_4 * (|x - mean| |rstd| |gamma| + |beta|).  Their contribution is
|alpha| * |A| . dB.
"""
import math

import torch

A_KC, A_MC, A_CONV, A_PATCH = 0, 1, 2, 3
B_KC, B_NC, B_CONVW, B_NC_GELU, B_NC_LN, B_PATCHT = 0, 1, 2, 3, 4, 5
ACT_NONE, ACT_GELU, ACT_RELU, ACT_MUL_DGELU, ACT_MUL_DRELU = 0, 1, 2, 3, 4
OUT_STRIDED, OUT_CONVT2X, OUT_PATCH = 0, 1, 2

U = 2.0 ** -24
EPILOGUE_ROUNDINGS = 5
GELU_LIPSCHITZ = 1.1289041452           # max |GELU'(x)| = Phi(sqrt 2) + sqrt 2 phi(sqrt 2)
ERF_GELU_REL = 7.1e-7                   # 2 x the measured 3.53e-7 (see the module docstring)
ERF_DGELU_ABS = 5.5e-7                  # 2 x the measured 2.74e-7


def gamma(n):
    return n * U / (1.0 - n * U)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def operand(t, ld=0, off=0, bso=0, bsi=0):
    return {"t": t, "ld": ld, "off": off, "bso": bso, "bsi": bsi}


def conv(H, W, C1, KH=1, KW=1, dil=1, pad=0, sign=1, C2=0, rep=1, src2=None, src2_off=0, ld2=0, patch=0, stride=1, Ho=0,
         Wo=0):
    return dict(H=H, W=W, Ho=Ho, Wo=Wo, stride=stride, C1=C1, C2=C2, rep=rep, KH=KH, KW=KW, dil=dil, pad=pad, sign=sign,
                src2=src2, src2_off=src2_off, ld2=ld2, patch=patch)


def desc(**kw):
    """A descriptor dict with the header's defaults.  Pointers are (buffer name, element offset) pairs."""
    d = dict(a_mode=A_KC, b_mode=B_KC, M=0, N=0, K=0, batch=1, batch_inner=1, ksplit=0, A=None, B=None, conv=None,
             C="C", c_off=0, out_mode=OUT_STRIDED, ldc_m=None, ldc_n=1, c_bso=0, c_bsi=0, ct=(0, 0, 0),
             alpha=1.0, bias=None, bias_mod=0, act=ACT_NONE, preact=None, p_off=0,
             resid=None, r_off=0, ldr_m=None, ldr_n=1, r_bso=0, r_bsi=0, accumulate=False,
             b_stats=None, b_gamma=None, b_beta=None)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw)
    if d["ldc_m"] is None:
        d["ldc_m"] = d["N"]
    if d["ldr_m"] is None:
        d["ldr_m"] = d["ldc_m"]
    return d


def _src(tensors, name):
    return tensors[name].detach().to("cpu", torch.float64).reshape(-1)


def _gather(src, idx, valid=None):
    """src[idx] where valid, 0 elsewhere; an address outside the buffer at a valid position is a mistake of the caller."""
    if valid is None:
        valid = torch.ones_like(idx, dtype=torch.bool)
    idx, valid = torch.broadcast_tensors(idx, valid)
    if valid.any():
        lo, hi = int(idx[valid].min()), int(idx[valid].max())
        assert 0 <= lo and hi < src.numel(), ("operand address outside its buffer", lo, hi, src.numel())
    return torch.where(valid, src[idx.clamp(0, src.numel() - 1)], torch.zeros((), dtype=src.dtype))


def _conv_gather(cv, tensors, op, pix, kk):
    """Implicit im2col element: output pixel index `pix` = (img, oh, ow), reduction index `kk` = (tap, ci)."""
    H, W = cv["H"], cv["W"]
    Ho, Wo = cv["Ho"] or H, cv["Wo"] or W
    s = max(cv["stride"], 1)
    C1, C2 = cv["C1"], cv["C2"]
    ow, t = pix % Wo, pix // Wo
    oh, img = t % Ho, t // Ho
    tap, ci = kk // (C1 + C2), kk % (C1 + C2)
    ti, tj = tap // cv["KW"], tap % cv["KW"]
    ih = oh * s + cv["sign"] * (ti * cv["dil"] - cv["pad"])
    iw = ow * s + cv["sign"] * (tj * cv["dil"] - cv["pad"])
    inside = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    v = _gather(_src(tensors, op["t"]), op["off"] + ((img * H + ih) * W + iw) * op["ld"] + ci, inside & (ci < C1))
    if C2 > 0:
        a2 = cv["src2_off"] + (((img // cv["rep"]) * H + ih) * W + iw) * cv["ld2"] + (ci - C1)
        v = v + _gather(_src(tensors, cv["src2"]), a2, inside & (ci >= C1))
    return v


def _patch_gather(cv, tensors, op, tok, kk):
    """Patch element: token `tok` = (img, py, px) on the ceil(H/P) x ceil(W/P) grid, `kk` = (c, i, j); NCHW image; pixels
    past the bottom / right edge read 0."""
    P, H, W, C1 = cv["patch"], cv["H"], cv["W"], cv["C1"]
    npx, npy = -(-W // P), -(-H // P)
    px, t = tok % npx, tok // npx
    py, img = t % npy, t // npy
    c, r2 = kk // (P * P), kk % (P * P)
    i, j = r2 // P, r2 % P
    y, x = py * P + i, px * P + j
    return _gather(_src(tensors, op["t"]), op["off"] + ((img * C1 + c) * H + y) * W + x, (y < H) & (x < W))


def _zoff(d, bso, bsi):
    z = torch.arange(d["batch"])
    return (z // d["batch_inner"]) * bso + (z % d["batch_inner"]) * bsi


def logical_A(d, tensors):
    """A[z][m][k] as float64, z over the operand batch (one slab when split-K ignores the batch strides)."""
    M, K, op = d["M"], d["K"], d["A"]
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    zo = torch.zeros(1, dtype=torch.long) if d["ksplit"] > 0 else _zoff(d, op["bso"], op["bsi"])
    mode = d["a_mode"]
    if mode == A_KC:
        return _gather(_src(tensors, op["t"]), op["off"] + zo[:, None, None] + (m * op["ld"] + k)[None])
    if mode == A_MC:
        return _gather(_src(tensors, op["t"]), op["off"] + zo[:, None, None] + (k * op["ld"] + m)[None])
    assert d["batch"] == 1 or d["ksplit"] > 0, "conv / patch operands are unbatched"
    if mode == A_CONV:
        return _conv_gather(d["conv"], tensors, op, m, k)[None]
    if mode == A_PATCH:
        return _patch_gather(d["conv"], tensors, op, m, k)[None]
    raise ValueError(f"a_mode {mode}")


def logical_B(d, tensors):
    """(B[z][n][k], dB[z][n][k]): the operand and the a-priori error of the elements a producer computes in fp32."""
    N, K, op = d["N"], d["K"], d["B"]
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    zo = torch.zeros(1, dtype=torch.long) if d["ksplit"] > 0 else _zoff(d, op["bso"], op["bsi"])
    mode = d["b_mode"]
    if mode == B_KC:
        return _gather(_src(tensors, op["t"]), op["off"] + zo[:, None, None] + (n * op["ld"] + k)[None]), None
    if mode == B_NC:
        return _gather(_src(tensors, op["t"]), op["off"] + zo[:, None, None] + (k * op["ld"] + n)[None]), None
    assert d["batch"] == 1 or d["ksplit"] > 0, "conv / producer operands are unbatched"
    if mode == B_CONVW:
        return _conv_gather(d["conv"], tensors, op, k, n)[None], None
    if mode == B_PATCHT:
        return _patch_gather(d["conv"], tensors, op, k, n)[None], None
    x = _gather(_src(tensors, op["t"]), op["off"] + k * op["ld"] + n)
    if mode == B_NC_GELU:
        g = gelu64(x)
        return g[None], (ERF_GELU_REL * x.abs())[None]
    if mode == B_NC_LN:
        st = _src(tensors, d["b_stats"])
        mean, rstd = st[2 * k], st[2 * k + 1]
        ga, be = _src(tensors, d["b_gamma"])[n], _src(tensors, d["b_beta"])[n]
        y = (x - mean) * rstd * ga + be
        return y[None], (gamma(4) * ((x - mean).abs() * rstd.abs() * ga.abs() + be.abs()))[None]
    raise ValueError(f"b_mode {mode}")


def out_index(d, z, what="C"):
    """Element offsets [M, N] (from the buffer start) of slab z in the output / preact / resid addressing."""
    M, N = d["M"], d["N"]
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    zo, zi = z // d["batch_inner"], z % d["batch_inner"]
    if what == "R":
        off, ldm, ldn, bo, bi = d["r_off"], d["ldr_m"], d["ldr_n"], d["r_bso"], d["r_bsi"]
    else:
        off, ldm, ldn, bo, bi = d["c_off"] if what == "C" else d["p_off"], d["ldc_m"], d["ldc_n"], d["c_bso"], d["c_bsi"]
    mode = d["out_mode"]
    if mode == OUT_STRIDED:
        return off + zo * bo + zi * bi + m * ldm + n * ldn
    assert d["batch"] == 1, "the scatter outputs are unbatched"
    if mode == OUT_CONVT2X:
        assert what == "C", "preact / resid are not defined for SVL_OUT_CONVT2X"
        Hc, Wc, Co = d["ct"]
        assert N == 4 * Co
        w, t = m % Wc, m // Wc
        h, img = t % Hc, t // Hc
        ab, co = n // Co, n % Co
        a, b = ab // 2, ab % 2
        return off + ((img * (2 * Hc) + 2 * h + a) * (2 * Wc) + 2 * w + b) * ldm + co
    if mode == OUT_PATCH:
        P = d["ct"][0]
        img, p = m // P, m % P
        if what == "R":   # the position embedding: row 1 + p, shared by the images
            return off + (1 + p) * ldm + n
        assert what == "C"
        return off + (img * (P + 1) + 1 + p) * ldm + n
    raise ValueError(f"out_mode {mode}")


class Result:
    __slots__ = ("C64", "written_mask", "bound", "P64", "p_mask", "p_bound")


def reference_full(d, tensors):
    """reference() plus the same three tensors for the `preact` buffer (None without one)."""
    M, N, K = d["M"], d["N"], d["K"]
    assert M > 0 and N > 0 and K >= 0 and d["batch"] >= 1 and d["batch_inner"] >= 1
    if d["ksplit"] > 0:
        assert d["ksplit"] * d["batch"] >= K
    A = logical_A(d, tensors)
    B, dB = logical_B(d, tensors)
    Cin = _src(tensors, d["C"])
    out, mask, bound = Cin.clone(), torch.zeros(Cin.numel(), dtype=torch.bool), torch.zeros_like(Cin)
    pre = pmask = pbound = None
    if d["preact"] is not None:
        assert d["out_mode"] == OUT_STRIDED
        pre = _src(tensors, d["preact"]).clone()
        pmask, pbound = torch.zeros(pre.numel(), dtype=torch.bool), torch.zeros_like(pre)
    bias = None
    if d["bias"] is not None:
        n = torch.arange(N)
        bias = _src(tensors, d["bias"])[n % d["bias_mod"] if d["bias_mod"] > 0 else n][None, :]
    resid = _src(tensors, d["resid"]) if d["resid"] is not None else None
    act, alpha = d["act"], float(d["alpha"])
    if act in (ACT_MUL_DGELU, ACT_MUL_DRELU):
        assert resid is not None and d["out_mode"] == OUT_STRIDED, "the backward activations read resid as z"
    for z in range(d["batch"]):
        k0, k1 = (z * d["ksplit"], min(K, (z + 1) * d["ksplit"])) if d["ksplit"] > 0 else (0, K)
        k0, k1 = min(k0, K), max(min(k0, K), k1)     # an empty range gives a zero slab
        zop = 0 if d["ksplit"] > 0 else z
        Az, Bz = A[zop][:, k0:k1], B[zop][:, k0:k1]
        acc = Az @ Bz.t()
        mag = abs(alpha) * (Az.abs() @ Bz.abs().t())
        prod = abs(alpha) * (Az.abs() @ dB[zop][:, k0:k1].t()) if dB is not None else 0.0
        g = gamma((k1 - k0) + EPILOGUE_ROUNDINGS)
        v = alpha * acc
        if bias is not None:
            v = v + bias
            mag = mag + bias.abs()
        err = g * mag + prod                      # |v_fp32 - v| so far
        if pre is not None:
            ip = out_index(d, z, "P").reshape(-1)
            assert not pmask[ip].any() and ip.unique().numel() == ip.numel(), "preact elements addressed twice"
            pre[ip], pmask[ip], pbound[ip] = v.reshape(-1), True, err.reshape(-1)
        if act == ACT_GELU:
            err = GELU_LIPSCHITZ * err + ERF_GELU_REL * (v.abs() + err)
            v = gelu64(v)
        elif act == ACT_RELU:
            v = v.clamp_min(0.0)
        if resid is not None:
            r = resid[out_index(d, z, "R")]
            if act == ACT_MUL_DGELU:
                err = GELU_LIPSCHITZ * err + ERF_DGELU_ABS * (v.abs() + err)
                v = v * dgelu64(r)
            elif act == ACT_MUL_DRELU:
                v = torch.where(r > 0, v, torch.zeros((), dtype=v.dtype))
            else:
                v = v + r
                err = err + g * r.abs()
        ic = out_index(d, z, "C").reshape(-1)
        assert 0 <= int(ic.min()) and int(ic.max()) < out.numel(), "output address outside its buffer"
        assert not mask[ic].any() and ic.unique().numel() == ic.numel(), "output elements addressed twice"
        v, err = v.reshape(-1), (err + torch.zeros_like(v)).reshape(-1)
        if d["accumulate"]:
            v = v + Cin[ic]
            err = err + g * Cin[ic].abs()
        out[ic], mask[ic], bound[ic] = v, True, err
    res = Result()
    res.C64, res.written_mask, res.bound = out, mask, bound
    res.P64, res.p_mask, res.p_bound = pre, pmask, pbound
    return res


def reference(d, tensors):
    """(C64, written_mask, bound): flat float64 copy of the output buffer with the descriptor's result scattered into it, the
    elements the descriptor addresses, and the componentwise a-priori error bound of an fp32 family (0 outside the mask)."""
    r = reference_full(d, tensors)
    return r.C64, r.written_mask, r.bound
