"""The descriptor table of svl_gemm_f32: one row per dispatch branch, with the svl_last_gemm_path() each row must take in
arithmetic modes 0 and 6, and the descriptors the entry point must refuse.  Rows are built from host tensors (fixed seeds,
fixed shapes): tests/test_gemm_desc_gpu.py launches them, tests/test_gemm_route_host.py asks svl_gemm_route about them."""
import ctypes as C

import torch

import gemm_desc_ref as R

SENT_BITS = 0x7FC0BEEF         # a quiet NaN with a payload: what every gap, guard and not-yet-written element holds


# ------------------------------------------------------------------------------------------------------ buffers
def sentinel(n):
    return torch.full((n,), SENT_BITS, dtype=torch.int32).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def padded(t, ld, off=0, tail=5):
    """[rows, cols] -> flat fp32 buffer: `off` elements in front, row pitch `ld`, `tail` behind; every gap is the sentinel."""
    rows, cols = t.shape
    buf = sentinel(off + rows * ld + tail).clone()
    buf[off:off + rows * ld].view(rows, ld)[:, :cols] = t
    return buf


def nhwc(x, ld, off=0):
    n, c, h, w = x.shape
    return padded(x.permute(0, 2, 3, 1).reshape(n * h * w, c), ld, off)


def outbuf(T, name, extent, pitch, odd=0, seed=99):
    """A buffer for an output of `extent` elements with a guard of >= one row (`pitch`) on both sides; returns the offset.
    The content is the C_in of accumulate rows; the runner overwrites whatever the descriptor does not read."""
    off = pitch + odd
    T[name] = rnd(off + extent + pitch + 3, seed=seed)
    return off


# ------------------------------------------------------------------------------------------------------ the table
class Row:
    def __init__(self, name, build, p0=0, p6=0, emu_h2=True):
        self.name, self.build, self.paths, self.emu_h2 = name, build, {0: p0, 6: p6}, emu_h2

    def __repr__(self):
        return self.name


ROWS = []


def row(name, p0=0, p6=0, emu_h2=True):
    def deco(fn):
        ROWS.append(Row(name, fn, p0, p6, emu_h2))
        return fn
    return deco


def dense(am, bm, M, N, K, a_pad=0, b_pad=0, a_off=0, b_off=0, c_pad=3, c_odd=1, seed=1, scale=1.0, **kw):
    """Dense descriptor on fresh operands; returns (d, T)."""
    a, b = rnd(M, K, seed=seed), rnd(N, K, seed=seed + 1) * scale
    lda = (K if am == R.A_KC else M) + a_pad
    ldb = (K if bm == R.B_KC else N) + b_pad
    T = {"A": padded(a if am == R.A_KC else a.t().contiguous(), lda, a_off),
         "B": padded(b if bm == R.B_KC else b.t().contiguous(), ldb, b_off)}
    ldc = N + c_pad
    c_off = outbuf(T, "C", M * ldc, ldc, c_odd)
    d = R.desc(a_mode=am, b_mode=bm, M=M, N=N, K=K, A=R.operand("A", lda, a_off), B=R.operand("B", ldb, b_off),
               ldc_m=ldc, c_off=c_off, **kw)
    return d, T


def epilogue(d, T, bias=True, bias_mod=0, resid=None, preact=False, seed=50):
    """Adds bias / resid ("row": padded row-major with an offset, "col": column-major) / preact to a strided descriptor."""
    M, N = d["M"], d["N"]
    if bias:
        T["bias"] = rnd(bias_mod if bias_mod else N, seed=seed)
        d["bias"], d["bias_mod"] = "bias", bias_mod
    if resid == "row":
        T["R"] = padded(rnd(M, N, seed=seed + 1), N + 5, 3)
        d.update(resid="R", r_off=3, ldr_m=N + 5, ldr_n=1)
    elif resid == "col":
        T["R"] = padded(rnd(N, M, seed=seed + 1), M + 2, 1)
        d.update(resid="R", r_off=1, ldr_m=1, ldr_n=M + 2)
    if preact:
        d["preact"] = "P"
        d["p_off"] = outbuf(T, "P", M * d["ldc_m"], d["ldc_m"], 2, seed=seed + 2)
    return d, T


# 1. dense: four layout pairs x the five tile-shape branches, K cycling through {1, 5, 16, 70, 769}, operand pitch / offset
#    cycling through natural, padded by 4 (vector loads), padded by 3 (ld % 4 != 0) and pointers offset by 1 .. 3 elements
PAIRS = [("nt", R.A_KC, R.B_KC), ("nn", R.A_KC, R.B_NC), ("tt", R.A_MC, R.B_KC), ("tn", R.A_MC, R.B_NC)]
BRANCHES = [("m32", 20, 200), ("m64", 50, 150), ("n32", 300, 21), ("n64", 200, 50), ("gen", 257, 130)]
KS = [1, 5, 16, 70, 769]
VARIANTS = [dict(), dict(a_pad=4, b_pad=8), dict(a_pad=3, b_pad=1), dict(a_off=1, b_off=3), dict(a_off=2, b_off=0, a_pad=1)]
for pi, (pn, am, bm) in enumerate(PAIRS):
    for bi, (bn, M_, N_) in enumerate(BRANCHES):
        K_ = KS[(pi + bi) % 5]
        var = VARIANTS[(2 * pi + bi) % 5]
        split = bn == "gen" and K_ >= 64
        ROWS.append(Row(f"dense_{pn}_{bn}_K{K_}", (lambda am=am, bm=bm, M_=M_, N_=N_, K_=K_, var=var, s=10 * pi + bi:
                                                    dense(am, bm, M_, N_, K_, seed=100 + s, **var)), 0, 1 if split else 0))
# the general branch at the remaining K values, both alignments
for K_, var in [(1, dict()), (5, dict(a_off=3)), (16, dict(a_pad=4)), (70, dict(a_pad=2, b_pad=2)), (769, dict())]:
    ROWS.append(Row(f"dense_nt_gen2_K{K_}", (lambda K_=K_, var=var: dense(R.A_KC, R.B_KC, 300, 140, K_, seed=150 + K_, **var)),
                    0, 1 if K_ >= 64 else 0))


@row("dense_K0_epilogue_of_zero")
def _():
    d, T = dense(R.A_KC, R.B_KC, 70, 45, 0, seed=160, alpha=-0.37, act=R.ACT_RELU, accumulate=True)
    T["A"], T["B"] = sentinel(8).clone(), sentinel(8).clone()     # nothing of the operands may be read
    d["A"], d["B"] = R.operand("A", 0), R.operand("B", 0)
    return epilogue(d, T, resid="row")


# 2. output addressing and epilogue
@row("out_colmajor_cosine_store")
def _():
    M, N, K, HW = 529, 21, 70, 529
    d, T = dense(R.A_KC, R.B_KC, M, N, K, seed=200, alpha=-0.37)
    c_off = outbuf(T, "C", N * (HW + 6), HW + 6, 2)     # odd offset
    d.update(ldc_m=1, ldc_n=HW + 6, c_off=c_off)
    return d, T


def attention_layout(M, N, K, seed):
    zo, zi = 2, 3
    a, b, r = rnd(zo, M, zi, K, seed=seed), rnd(zi, zo, K, N, seed=seed + 1), rnd(zi, zo, N, M, seed=seed + 2)
    T = {"A": padded(a.reshape(zo * M, zi * K), zi * K, 4), "B": padded(b.reshape(zi * zo * K, N), N, 0),
         "R": padded(r.reshape(zi * zo * N, M), M, 2)}
    pitch = zi * N + 4
    c_off = outbuf(T, "C", zo * M * pitch, pitch, 1)
    d = R.desc(a_mode=R.A_KC, b_mode=R.B_NC, M=M, N=N, K=K, batch=6, batch_inner=3,
               A=R.operand("A", zi * K, 4, bso=M * zi * K, bsi=K), B=R.operand("B", N, 0, bso=K * N, bsi=zo * K * N),
               c_off=c_off, ldc_m=pitch, c_bso=M * pitch, c_bsi=N, alpha=-0.37,
               resid="R", r_off=2, ldr_m=1, ldr_n=M, r_bso=N * M, r_bsi=zo * N * M)
    return d, T


ROWS.append(Row("batch6_inner3_attention_small", lambda: attention_layout(50, 50, 16, 210)))
ROWS.append(Row("batch6_inner3_attention_split", lambda: attention_layout(260, 100, 64, 215), 0, 1))

ACTS = [("none", R.ACT_NONE), ("gelu", R.ACT_GELU), ("relu", R.ACT_RELU), ("dgelu", R.ACT_MUL_DGELU), ("drelu", R.ACT_MUL_DRELU)]
for ai, (an, act_) in enumerate(ACTS):
    # small (exact kernel in both modes), alternating the fast and the general epilogue (column-major resid)
    ROWS.append(Row(f"epi_{an}_small", (lambda act_=act_, ai=ai: epilogue(
        *dense(R.A_KC, R.B_NC, 70, 45, 33, seed=220 + ai, alpha=-0.37, act=act_, accumulate=ai % 2 == 0),
        bias_mod=15 if ai % 2 else 0, resid="col" if ai % 2 else "row", preact=True))))
    # above the mode-6 thresholds (split kernel's epilogue)
    ROWS.append(Row(f"epi_{an}_large", (lambda act_=act_, ai=ai: epilogue(
        *dense(R.A_KC, R.B_KC, 300, 100, 64, seed=230 + ai, alpha=-0.37, act=act_, accumulate=ai % 2 == 1),
        bias_mod=0 if ai % 2 else 25, resid="row" if ai % 2 else "col", preact=ai != 3)), 0, 1))


# 3. split-K: K not a multiple of ksplit, a short last slab, one trailing slab that is empty
def splitk(d, T, ks, batch):
    M, N = d["M"], d["N"]
    slab = M * d["ldc_m"] + 7
    c_off = outbuf(T, "C", batch * slab, d["ldc_m"], 1)
    d.update(ksplit=ks, batch=batch, c_bso=slab, c_off=c_off)
    d["A"]["bso"], d["B"]["bso"], d["A"]["bsi"] = 10 ** 7, 10 ** 7, 10 ** 7   # ignored under split-K
    return d, T


ROWS.append(Row("splitk_dense_small", lambda: splitk(*dense(R.A_MC, R.B_NC, 130, 70, 257, seed=300), 48, 7)))
ROWS.append(Row("splitk_dense_split", lambda: splitk(*dense(R.A_MC, R.B_NC, 260, 100, 300, seed=302), 64, 6), 0, 1))


def producer(mode, M, N, K, seed):
    d, T = dense(R.A_MC, R.B_NC, M, N, K, seed=seed, a_pad=4, b_pad=4, scale=2.0)
    d["b_mode"] = mode
    if mode == R.B_NC_LN:
        x = T["B"][:K * (N + 4)].view(K, N + 4)[:, :N].double()
        T["st"] = torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()], 1).reshape(-1).float()
        T["ga"], T["be"] = rnd(N, seed=seed + 5), rnd(N, seed=seed + 6)
        d.update(b_stats="st", b_gamma="ga", b_beta="be")
    return d, T


ROWS.append(Row("splitk_gelu_small", lambda: splitk(*producer(R.B_NC_GELU, 130, 70, 257, 310), 48, 7)))
ROWS.append(Row("splitk_gelu_split", lambda: splitk(*producer(R.B_NC_GELU, 260, 100, 300, 312), 64, 6), 0, 1))
ROWS.append(Row("splitk_ln_small", lambda: splitk(*producer(R.B_NC_LN, 130, 70, 257, 314), 48, 7)))
ROWS.append(Row("splitk_ln_split", lambda: splitk(*producer(R.B_NC_LN, 260, 100, 300, 316), 64, 6), 0, 1))
ROWS.append(Row("gelu_producer_unsplit", lambda: producer(R.B_NC_GELU, 70, 45, 33, 318)))


def patcht(n, Cc, H, W, P, E, ks, batch, seed):
    tok = -(-H // P) * -(-W // P)
    img, dy = rnd(n, Cc, H, W, seed=seed), rnd(n * tok, E, seed=seed + 1)
    T = {"img": torch.cat([img.reshape(-1), sentinel(5)]), "dy": padded(dy, E + 4)}
    d = R.desc(a_mode=R.A_MC, b_mode=R.B_PATCHT, M=E, N=Cc * P * P, K=n * tok, A=R.operand("dy", E + 4), B=R.operand("img"),
               conv=R.conv(H, W, Cc, patch=P), ldc_m=Cc * P * P + 4)
    return splitk(d, T, ks, batch)


ROWS.append(Row("splitk_patcht_ragged_small", lambda: patcht(2, 3, 40, 56, 16, 40, 8, 4, 320)))
ROWS.append(Row("splitk_patcht_ragged_split", lambda: patcht(6, 3, 40, 56, 16, 260, 32, 4, 322), 0, 1))
ROWS.append(Row("splitk_patcht_whole_patches", lambda: patcht(2, 3, 32, 48, 16, 40, 5, 3, 324)))


# 4. implicit-GEMM convolutions and their weight gradients
def conv_fwd(n, Ci, Co, H, W, k, dil, pad, stride=1, sign=1, ld_pad=0, x_off=0, C2=0, rep=1, seed=400, M=None, c_pad=4,
             **kw):
    Ho, Wo = ((H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1)
    if sign < 0:
        Ho, Wo = H, W
    x, w = rnd(n, Ci, H, W, seed=seed), rnd(Co, k * k * (Ci + C2), seed=seed + 1)
    T = {"x": nhwc(x, Ci + ld_pad, x_off), "w": padded(w, k * k * (Ci + C2))}
    geo = R.conv(H, W, Ci, KH=k, KW=k, dil=dil, pad=pad, sign=sign, stride=stride, Ho=Ho if stride > 1 else 0,
                 Wo=Wo if stride > 1 else 0)
    if C2:
        T["x2"] = nhwc(rnd(n // rep, C2, H, W, seed=seed + 2), C2 + 4, 8)
        geo.update(C2=C2, rep=rep, src2="x2", src2_off=8, ld2=C2 + 4)
    M = M or n * Ho * Wo
    ldc = Co + c_pad
    c_off = outbuf(T, "C", M * ldc, ldc, 0)
    d = R.desc(a_mode=R.A_CONV, M=M, N=Co, K=k * k * (Ci + C2), A=R.operand("x", Ci + ld_pad, x_off),
               B=R.operand("w", k * k * (Ci + C2)), conv=geo, ldc_m=ldc, c_off=c_off, **kw)
    return d, T


def conv_wgrad(n, Ci, Co, H, W, k, dil, pad, stride=1, ld_pad=0, x_off=0, C2=0, rep=1, seed=450, ks=0, batch=1):
    Ho, Wo = ((H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1)
    x, dy = rnd(n, Ci, H, W, seed=seed), rnd(n * Ho * Wo, Co, seed=seed + 1)
    T = {"x": nhwc(x, Ci + ld_pad, x_off), "dy": padded(dy, Co + 4)}
    geo = R.conv(H, W, Ci, KH=k, KW=k, dil=dil, pad=pad, stride=stride, Ho=Ho if stride > 1 else 0, Wo=Wo if stride > 1 else 0)
    if C2:
        T["x2"] = nhwc(rnd(n // rep, C2, H, W, seed=seed + 2), C2 + 4, 8)
        geo.update(C2=C2, rep=rep, src2="x2", src2_off=8, ld2=C2 + 4)
    N = k * k * (Ci + C2)
    d = R.desc(a_mode=R.A_MC, b_mode=R.B_CONVW, M=Co, N=N, K=n * Ho * Wo, A=R.operand("dy", Co + 4),
               B=R.operand("x", Ci + ld_pad, x_off), conv=geo, ldc_m=N + 4)
    if ks:
        return splitk(d, T, ks, batch)
    d["c_off"] = outbuf(T, "C", Co * (N + 4), N + 4, 0)
    return d, T


CONV_GEOMS = [  # name, n, Ci, Co, H, W, k, dil, pad, stride, extra
    ("k1", 2, 8, 40, 9, 7, 1, 1, 0, 1, dict()),
    ("k2s2_convT_backward", 2, 8, 12, 14, 10, 2, 1, 0, 2, dict()),
    ("k3", 2, 8, 40, 9, 11, 3, 1, 1, 1, dict()),
    ("k3_dil6", 1, 8, 24, 13, 13, 3, 6, 6, 1, dict()),
    ("k3_dil_beyond_image", 1, 8, 24, 9, 9, 3, 20, 20, 1, dict()),
    ("k7s2_stem_odd", 2, 3, 32, 37, 29, 7, 1, 3, 2, dict(ld_pad=2)),
    ("k3s2_odd", 1, 4, 20, 15, 21, 3, 1, 1, 2, dict()),
    ("k3_c5_ld7_offset", 2, 5, 40, 10, 9, 3, 1, 1, 1, dict(ld_pad=2, x_off=1)),
    ("k3_two_sources_rep3", 6, 5, 40, 10, 10, 3, 1, 1, 1, dict(ld_pad=2, C2=8, rep=3)),
    ("k3_two_sources_aligned", 6, 4, 40, 10, 10, 3, 2, 2, 1, dict(C2=8, rep=3)),
]
for gi, (gn, n_, Ci_, Co_, H_, W_, k_, dil_, pad_, st_, ex_) in enumerate(CONV_GEOMS):
    ROWS.append(Row(f"conv_fwd_{gn}", (lambda a=(n_, Ci_, Co_, H_, W_, k_, dil_, pad_, st_), ex_=ex_, gi=gi: epilogue(
        *conv_fwd(*a, seed=400 + gi, act=R.ACT_RELU if gi % 2 else R.ACT_NONE, **ex_)))))
    ROWS.append(Row(f"conv_wgrad_{gn}", (lambda a=(n_, Ci_, Co_, H_, W_, k_, dil_, pad_, st_), ex_=ex_, gi=gi: conv_wgrad(
        *a, seed=450 + gi, ks=37 if gi % 2 else 0, batch=-(-(a[0] * a[3] * a[4]) // 37) if gi % 2 else 1, **ex_))))
ROWS.append(Row("conv_dgrad_k3_dil2", lambda: conv_fwd(2, 12, 20, 9, 11, 3, 2, 2, sign=-1, seed=470, accumulate=True)))
ROWS.append(Row("conv_dgrad_k7", lambda: conv_fwd(1, 6, 3, 12, 10, 7, 1, 3, sign=-1, seed=472, ld_pad=1)))
# Conv2d(1 -> 16), 3 x 3, on both sides of M = 32768: implicit GEMM below, the elementwise kernel from there on
ROWS.append(Row("conv_cin1_M32767", lambda: epilogue(*conv_fwd(2, 1, 16, 128, 128, 3, 1, 1, seed=474, M=32767, ld_pad=0,
                                                               act=R.ACT_RELU))))
ROWS.append(Row("conv_cin1_M32768", lambda: epilogue(*conv_fwd(2, 1, 16, 128, 128, 3, 1, 1, seed=476, act=R.ACT_RELU)), 3, 3))
# mode-6 conditions of the implicit GEMM: K % 16, 16-byte alignment
ROWS.append(Row("conv6_K144", lambda: conv_fwd(1, 16, 96, 17, 17, 3, 2, 2, seed=480), 0, 1))
ROWS.append(Row("conv6_K108_not_16", lambda: conv_fwd(1, 12, 96, 17, 17, 3, 2, 2, seed=482), 0, 0))
ROWS.append(Row("conv6_unaligned_source", lambda: conv_fwd(1, 16, 96, 17, 17, 3, 2, 2, seed=484, x_off=1), 0, 0))
ROWS.append(Row("conv6_dgrad_K144", lambda: conv_fwd(1, 16, 96, 17, 17, 3, 2, 2, sign=-1, seed=486), 0, 1))
# ... and of its weight gradient: K = 1008 / 1024 pixels, Wo % 8, split-K with a short last slab and an empty one
ROWS.append(Row("wgrad6_K1008", lambda: conv_wgrad(1, 16, 96, 126, 8, 3, 1, 1, seed=490), 0, 0))
ROWS.append(Row("wgrad6_K1024", lambda: conv_wgrad(1, 16, 96, 128, 8, 3, 1, 1, seed=492), 0, 1))
ROWS.append(Row("wgrad6_splitk_Wo24", lambda: conv_wgrad(2, 16, 96, 24, 24, 3, 1, 1, seed=494, ks=256, batch=6), 0, 1))
ROWS.append(Row("wgrad6_splitk_Wo28", lambda: conv_wgrad(2, 16, 96, 24, 28, 3, 1, 1, seed=496, ks=256, batch=7), 0, 0))
ROWS.append(Row("wgrad6_s2_k2", lambda: conv_wgrad(2, 16, 96, 48, 32, 2, 1, 0, stride=2, seed=498), 0, 0))   # N = 64 < 96


# 5. patch embedding: gather + token scatter with the position embedding as resid; class-token rows are not addressed
def patch_embed(n, Cc, H, W, P, E, seed):
    tok = -(-H // P) * -(-W // P)
    img, w, pos = rnd(n, Cc, H, W, seed=seed), rnd(E, Cc * P * P, seed=seed + 1), rnd(tok + 1, E, seed=seed + 2)
    T = {"img": torch.cat([img.reshape(-1), sentinel(5)]), "w": padded(w, Cc * P * P), "pos": padded(pos, E + 4, 4),
         "bias": rnd(E, seed=seed + 3)}
    pitch = E + 4
    c_off = outbuf(T, "C", n * (tok + 1) * pitch, pitch, 0)
    d = R.desc(a_mode=R.A_PATCH, M=n * tok, N=E, K=Cc * P * P, A=R.operand("img"), B=R.operand("w", Cc * P * P),
               conv=R.conv(H, W, Cc, patch=P), out_mode=R.OUT_PATCH, ct=(tok, 0, 0), c_off=c_off, ldc_m=pitch,
               resid="pos", r_off=4, ldr_m=E + 4, bias="bias")
    return d, T


ROWS.append(Row("patch_embed_64", lambda: patch_embed(2, 3, 64, 64, 16, 40, 500)))
ROWS.append(Row("patch_embed_ragged_50x37", lambda: patch_embed(2, 3, 50, 37, 16, 40, 504)))
ROWS.append(Row("patch_embed_ragged_wide", lambda: patch_embed(3, 3, 72, 100, 16, 300, 508)))


# 6. ConvTranspose2d(k 2, s 2) pixel-shuffle store with bias[n % Cout]
def convT(n, H, W, Ci, Co, seed, **kw):
    x, w = rnd(n * H * W, Ci, seed=seed), rnd(4 * Co, Ci, seed=seed + 1)
    T = {"x": padded(x, Ci + 4), "w": padded(w, Ci), "bias": rnd(Co, seed=seed + 2)}
    pitch = Co + 4
    c_off = outbuf(T, "C", n * 4 * H * W * pitch, pitch * 2 * W, 0)
    d = R.desc(M=n * H * W, N=4 * Co, K=Ci, A=R.operand("x", Ci + 4), B=R.operand("w", Ci), out_mode=R.OUT_CONVT2X,
               ldc_m=pitch, c_off=c_off, ct=(H, W, Co), bias="bias", bias_mod=Co, **kw)
    return d, T


ROWS.append(Row("convT_small_general", lambda: convT(2, 10, 9, 64, 24, 600, act=R.ACT_RELU)))
ROWS.append(Row("convT_M32768_K64", lambda: convT(2, 128, 128, 64, 24, 602), 2, 1))
ROWS.append(Row("convT_M33024_K128", lambda: convT(2, 128, 129, 128, 24, 604, act=R.ACT_GELU), 2, 1))
ROWS.append(Row("convT_M33024_K64_accumulate", lambda: convT(2, 128, 129, 64, 24, 606, accumulate=True, alpha=-0.37), 2, 2))
ROWS.append(Row("convT_M32768_K192", lambda: convT(2, 128, 128, 192, 24, 608), 0, 0))

# 7. mode-6 thresholds of the dense launches, one row on each side
for nm, M_, N_, K_, p6 in [("M255", 255, 130, 70, 0), ("M256", 256, 130, 70, 1), ("N95", 300, 95, 70, 0), ("N96", 300, 96, 70, 1),
                           ("K48", 300, 130, 48, 0), ("K64", 300, 130, 64, 1)]:
    ROWS.append(Row(f"thr6_{nm}", (lambda M_=M_, N_=N_, K_=K_: dense(R.A_KC, R.B_KC, M_, N_, K_, seed=700 + M_ + N_ + K_)), 0, p6))
# an unaligned dense operand stays on the split kernel (its loaders fall back to 4-byte loads)
ROWS.append(Row("thr6_dense_unaligned", lambda: dense(R.A_KC, R.B_NC, 300, 130, 70, seed=710, a_off=1, b_pad=1), 0, 1))
# short-K row stream: K = 64 / 128 stream in mode 0; in mode 6 K = 64 streams on the split pipe, K = 128 joins the split kernel
for K_, p0, p6 in [(64, 2, 1), (128, 2, 1), (192, 0, 1)]:
    ROWS.append(Row(f"shortk_K{K_}", (lambda K_=K_: epilogue(*dense(R.A_KC, R.B_KC, 32768, 96, K_, seed=720 + K_, a_pad=4, c_pad=4,
                                                                   c_odd=0, act=R.ACT_GELU))), p0, p6))
ROWS.append(Row("shortk_K64_resid_general_epilogue", lambda: epilogue(
    *dense(R.A_KC, R.B_KC, 32800, 100, 64, seed=730, c_pad=4, c_odd=0), resid="row"), 2, 2))
ROWS.append(Row("shortk_K64_M32767_below", lambda: dense(R.A_KC, R.B_KC, 32767, 96, 64, seed=732, c_pad=4, c_odd=0), 0, 1))
# ragged token count: the leftover rows run as a second launch on the helper stream
ROWS.append(Row("ragged_fork_M8200", lambda: epilogue(*dense(R.A_KC, R.B_KC, 8200, 768, 768, seed=740, scale=0.05,
                                                             act=R.ACT_GELU), resid="row", preact=True), 0, 1, emu_h2=False))
# the fp16 x 2 form (emu_ws given, >= 4 GFLOP) next to the same row without emu_ws
for nm, h2 in [("h2", True), ("bf16x3", False)]:
    ROWS.append(Row(f"big_dense_{nm}", lambda: dense(R.A_KC, R.B_KC, 1282, 1300, 1320, seed=750, scale=0.05), 0, 4 if h2 else 1, h2))
    ROWS.append(Row(f"big_conv_fwd_{nm}", lambda: conv_fwd(1, 128, 128, 120, 120, 3, 2, 2, seed=752), 0, 4 if h2 else 1, h2))
    ROWS.append(Row(f"big_conv_wgrad_{nm}", lambda: conv_wgrad(1, 128, 128, 120, 120, 3, 2, 2, seed=754, ks=2048, batch=8),
                    0, 4 if h2 else 1, h2))

assert len({r.name for r in ROWS}) == len(ROWS)



# ------------------------------------------------------------------------------------------------------ descriptors
def gemm_args(d, Td):
    """(args, kwargs) of ops.gemm / ops.gemm_desc for a dict descriptor on the buffers Td (host or device tensors)."""
    from semivl_amd import ops

    def view(name, off=0):
        return None if name is None else Td[name][off:]

    g = None
    cv = d["conv"]
    if cv is not None:
        g = ops.conv_geom(cv["H"], cv["W"], cv["C1"], cv["KH"], cv["KW"], dil=cv["dil"], pad=cv["pad"], sign=cv["sign"],
                          C2=cv["C2"], rep=cv["rep"], src2=view(cv["src2"], cv["src2_off"]), ld2=cv["ld2"],
                          patch=cv["patch"], stride=cv["stride"], Ho=cv["Ho"], Wo=cv["Wo"])
    A, B = d["A"], d["B"]
    b_aux = None if d["b_stats"] is None else (Td[d["b_stats"]], Td[d["b_gamma"]], Td[d["b_beta"]])
    args = (d["a_mode"], d["b_mode"], d["M"], d["N"], d["K"], ops.Op(Td[A["t"]], A["ld"], A["off"], A["bso"], A["bsi"]),
            ops.Op(Td[B["t"]], B["ld"], B["off"], B["bso"], B["bsi"]), Td[d["C"]])
    kw = dict(c_off=d["c_off"], ldc_m=d["ldc_m"],
              ldc_n=d["ldc_n"], batch=d["batch"], batch_inner=d["batch_inner"], ksplit=d["ksplit"], c_bso=d["c_bso"],
              c_bsi=d["c_bsi"], alpha=d["alpha"], bias=view(d["bias"]), bias_mod=d["bias_mod"], act=d["act"],
              resid=view(d["resid"]), r_off=d["r_off"], ldr_m=d["ldr_m"], ldr_n=d["ldr_n"], r_bso=d["r_bso"], r_bsi=d["r_bsi"],
              accumulate=d["accumulate"], out_mode=d["out_mode"], conv=g, ct=d["ct"], preact=view(d["preact"], d["p_off"]),
              b_aux=b_aux)
    return args, kw


def route(d, Td, emu_h2):
    """svl_gemm_route on the descriptor ops.gemm would launch: a dummy non-null emu_ws where ops.gemm would pass one."""
    from semivl_amd import ops
    args, kw = gemm_args(d, Td)
    c = ops.gemm_desc(*args, **kw)
    if ops.wants_emu_ws(c, emu_h2):
        c.emu_ws = C.c_void_p(16)
    return ops.gemm_route(c)


# ------------------------------------------------------------------------------------------------------ refusals
def cdesc(d, Td):
    """The ctypes descriptor of a dict descriptor (ops.gemm raises on a refusal; here the status itself is the subject)."""
    from semivl_amd import lib as L

    def ptr(name, off=0):
        return None if name is None else C.c_void_p(Td[name].data_ptr() + 4 * off)

    c = L.GemmDesc()
    c.a_mode, c.b_mode, c.M, c.N, c.K = d["a_mode"], d["b_mode"], d["M"], d["N"], d["K"]
    c.batch, c.batch_inner, c.ksplit = d["batch"], d["batch_inner"], d["ksplit"]
    for op, o in ((c.A, d["A"]), (c.B, d["B"])):
        op.ptr, op.ld, op.bs_outer, op.bs_inner = ptr(o["t"], o["off"]), o["ld"], o["bso"], o["bsi"]
    cv = d["conv"]
    if cv is not None:
        g = c.conv
        g.H, g.W, g.Ho, g.Wo, g.stride, g.C1, g.C2, g.rep = (cv[k] for k in ("H", "W", "Ho", "Wo", "stride", "C1", "C2", "rep"))
        g.KH, g.KW, g.dil, g.pad, g.sign, g.ld2, g.patch = (cv[k] for k in ("KH", "KW", "dil", "pad", "sign", "ld2", "patch"))
        g.src2 = ptr(cv["src2"], cv["src2_off"])
    c.C, c.out_mode = ptr(d["C"], d["c_off"]), d["out_mode"]
    c.ldc_m, c.ldc_n, c.c_bs_outer, c.c_bs_inner = d["ldc_m"], d["ldc_n"], d["c_bso"], d["c_bsi"]
    c.ct_H, c.ct_W, c.ct_Cout = d["ct"]
    c.alpha, c.bias, c.bias_mod, c.act = d["alpha"], ptr(d["bias"]), d["bias_mod"], d["act"]
    c.preact, c.resid = ptr(d["preact"], d["p_off"]), ptr(d["resid"], d["r_off"])
    c.ldr_m, c.ldr_n, c.r_bs_outer, c.r_bs_inner = d["ldr_m"], d["ldr_n"], d["r_bso"], d["r_bsi"]
    c.accumulate = 1 if d["accumulate"] else 0
    c.b_stats, c.b_gamma, c.b_beta = ptr(d["b_stats"]), ptr(d["b_gamma"]), ptr(d["b_beta"])
    return c


def refusals():
    def base():
        return epilogue(*dense(R.A_MC, R.B_NC, 40, 48, 30, seed=800), resid="row", preact=True)

    def ksplit_too_small():
        d, T = base()
        d.update(ksplit=7, batch=4)
        return d, T

    def batched_conv():
        d, T = conv_fwd(2, 8, 40, 9, 11, 3, 1, 1, seed=802)
        d.update(batch=2, c_bso=0)
        return d, T

    def preact_scatter():
        d, T = convT(2, 10, 9, 64, 24, 804)
        d["preact"], d["p_off"] = "C", d["c_off"]
        return d, T

    def producer_needs_mcontig():
        d, T = producer(R.B_NC_GELU, 40, 48, 30, 806)
        d["a_mode"] = R.A_KC
        return d, T

    def convT_bad_N():
        d, T = convT(2, 10, 9, 64, 24, 808)
        d["ct"] = (10, 9, 23)
        return d, T

    def batch_too_large():
        d, T = base()
        d.update(batch=65536, c_bso=0)
        return d, T

    def bad_mode_pair():
        d, T = conv_wgrad(2, 8, 40, 9, 11, 3, 1, 1, seed=810)
        d["a_mode"] = R.A_KC
        return d, T

    def convT_resid():
        d, T = convT(2, 10, 9, 64, 24, 812)
        T["R"] = rnd(T["C"].numel(), seed=813)
        d.update(resid="R", r_off=d["c_off"])
        return d, T

    def batched_patch_scatter():
        d, T = patch_embed(2, 3, 64, 64, 16, 40, 814)
        d.update(batch=2)
        return d, T

    return [("ksplit * batch < K", ksplit_too_small, -1), ("batched conv without split-K", batched_conv, -1),
            ("preact with a scatter output", preact_scatter, -1), ("B producer with A != MCONTIG", producer_needs_mcontig, -1),
            ("CONVT2X with N != 4 Cout", convT_bad_N, -1), ("batch > 65535", batch_too_large, -1),
            ("unsupported mode pair", bad_mode_pair, -3), ("resid with CONVT2X", convT_resid, -3),
            ("batched scatter output", batched_patch_scatter, -1)]
