"""The float64 restatement of svl_gemm_desc (tests/gemm_desc_ref.py) against independent torch float64 operations.

No GPU: the reference that the kernels are held to (tests/test_gemm_desc_gpu.py) is itself checked here on small ragged
cases.  Both sides are float64 sums of the same terms in a different order, so they agree to float64 rounding
(<= 1e-12 relative to the largest element)."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_desc_ref as R

F64 = torch.float64


def rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=F64)


def same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-300)
    assert float((got - want).abs().max()) <= 1e-12 * scale, float((got - want).abs().max()) / scale


def padded(t, ld, off=0, tail=3, fill=float("nan")):
    """[rows, cols] -> flat buffer with `off` elements in front, row pitch `ld`, `tail` behind; gaps hold `fill`."""
    rows, cols = t.shape
    buf = torch.full((off + rows * ld + tail,), fill, dtype=F64)
    buf[off:off + rows * ld].view(rows, ld)[:, :cols] = t
    return buf


def run(d, T):
    C64, mask, bound = R.reference(d, T)
    assert mask.dtype == torch.bool and C64.dtype == F64 and bound.shape == C64.shape
    assert bool((bound[~mask] == 0).all()) and bool((bound[mask] >= 0).all())
    keep = T[d["C"]].to(F64).reshape(-1)
    untouched = ~mask
    assert torch.equal(C64[untouched].nan_to_num(nan=7.0), keep[untouched].nan_to_num(nan=7.0)), "wrote outside the mask"
    return C64, mask


# ---------------------------------------------------------------------------------------------------------- dense
@pytest.mark.parametrize("a_mode,b_mode", [(R.A_KC, R.B_KC), (R.A_KC, R.B_NC), (R.A_MC, R.B_KC), (R.A_MC, R.B_NC)])
@pytest.mark.parametrize("M,N,K", [(5, 7, 11), (33, 2, 1), (3, 9, 0)])
def test_dense_layouts(a_mode, b_mode, M, N, K):
    a, b = rnd(M, K, seed=1), rnd(N, K, seed=2)
    A = padded(a if a_mode == R.A_KC else a.t().contiguous(), (K if a_mode == R.A_KC else M) + 3, off=2)
    B = padded(b if b_mode == R.B_KC else b.t().contiguous(), (K if b_mode == R.B_KC else N) + 1, off=1)
    d = R.desc(a_mode=a_mode, b_mode=b_mode, M=M, N=N, K=K, A=R.operand("A", (K if a_mode == R.A_KC else M) + 3, 2),
               B=R.operand("B", (K if b_mode == R.B_KC else N) + 1, 1), ldc_m=N + 2, c_off=5)
    T = {"A": A, "B": B, "C": torch.full((5 + M * (N + 2) + 4,), float("nan"), dtype=F64)}
    C64, mask = run(d, T)
    same(C64[5:5 + M * (N + 2)].view(M, N + 2)[:, :N], a @ b.t())
    want = torch.zeros(M, N + 2, dtype=torch.bool)
    want[:, :N] = True
    assert torch.equal(mask[5:5 + M * (N + 2)].view(M, N + 2), want) and int(mask.sum()) == M * N


def test_batch_outer_inner_strides():
    """batch = 6, batch_inner = 3 with distinct outer / inner strides on both operands, the output and resid (the attention
    layouts): einsum over (zo, zi)."""
    M, N, K, zo, zi = 4, 5, 6, 2, 3
    a, b, r = rnd(zo, zi, M, K, seed=3), rnd(zo, zi, K, N, seed=4), rnd(zi, zo, N, M, seed=5)
    # A: [zo][m][zi][k] (heads interleaved inside a token row); B: [zi][zo][k][n]; C: [zo][m][zi][n]; resid: [zi][zo][n][m]
    A = a.permute(0, 2, 1, 3).contiguous()
    B = b.permute(1, 0, 2, 3).contiguous()
    d = R.desc(a_mode=R.A_KC, b_mode=R.B_NC, M=M, N=N, K=K, batch=6, batch_inner=3,
               A=R.operand("A", zi * K, 0, bso=M * zi * K, bsi=K), B=R.operand("B", N, 0, bso=K * N, bsi=zo * K * N),
               ldc_m=zi * N, c_bso=M * zi * N, c_bsi=N, alpha=-0.37,
               resid="R", ldr_m=1, ldr_n=M, r_bso=N * M, r_bsi=zo * N * M)
    T = {"A": A.reshape(-1), "B": B.reshape(-1), "R": r.reshape(-1), "C": torch.zeros(zo * M * zi * N, dtype=F64)}
    C64, mask = run(d, T)
    want = -0.37 * torch.einsum("oimk,oikn->oimn", a, b) + r.permute(1, 0, 3, 2)
    same(C64.view(zo, M, zi, N), want.permute(0, 2, 1, 3))
    assert bool(mask.all())


@pytest.mark.parametrize("K,ks,batch", [(37, 8, 5), (37, 16, 3), (37, 5, 11), (16, 16, 1), (0, 4, 2)])
def test_split_k_slabs(K, ks, batch):
    """Slab z holds the partial product over [z ks, min(K, (z+1) ks)): a short last slab, and slabs past K are zero."""
    M, N = 6, 5
    a, b = rnd(K, M, seed=6), rnd(K, N, seed=7)
    d = R.desc(a_mode=R.A_MC, b_mode=R.B_NC, M=M, N=N, K=K, batch=batch, ksplit=ks,
               A=R.operand("A", M, 0, bso=10 ** 6, bsi=10 ** 6), B=R.operand("B", N, 0, bso=10 ** 6), c_bso=M * N + 3)
    T = {"A": a.reshape(-1), "B": b.reshape(-1), "C": torch.full((batch * (M * N + 3),), float("nan"), dtype=F64)}
    C64, mask = run(d, T)
    got = C64.view(batch, M * N + 3)[:, :M * N].reshape(batch, M, N)
    for z in range(batch):
        lo, hi = min(z * ks, K), min(K, (z + 1) * ks)
        same(got[z], torch.einsum("km,kn->mn", a[lo:hi], b[lo:hi]))
    same(got.sum(0), a.t() @ b)
    assert int(mask.sum()) == batch * M * N


# ---------------------------------------------------------------------------------------------------------- convolution
def nhwc(x, ld, off=0):
    n, c, h, w = x.shape
    return padded(x.permute(0, 2, 3, 1).reshape(n * h * w, c), ld, off)


CONV_CASES = [  # n, Ci, Co, H, W, k, dil, pad, stride
    (2, 3, 4, 7, 5, 1, 1, 0, 1), (1, 5, 3, 6, 9, 2, 1, 0, 2), (2, 3, 5, 9, 7, 3, 1, 1, 1), (1, 4, 2, 11, 9, 3, 6, 6, 1),
    (1, 2, 3, 5, 4, 3, 7, 7, 1), (2, 3, 4, 11, 9, 7, 1, 3, 2), (1, 3, 6, 9, 13, 3, 1, 1, 2), (1, 2, 2, 7, 7, 2, 1, 0, 2)]


@pytest.mark.parametrize("n,Ci,Co,H,W,k,dil,pad,stride", CONV_CASES)
def test_conv_forward_dgrad_wgrad(n, Ci, Co, H, W, k, dil, pad, stride):
    x = rnd(n, Ci, H, W, seed=8).requires_grad_(True)
    w = rnd(Co, Ci, k, k, seed=9).requires_grad_(True)
    bias = rnd(Co, seed=10)
    y = F.conv2d(x, w, bias, stride=stride, padding=pad, dilation=dil)
    Ho, Wo = y.shape[2:]
    dy = rnd(n, Co, Ho, Wo, seed=11)
    gx, gw = torch.autograd.grad(y, (x, w), dy)
    ldx, ldy, K = Ci + 3, Co + 1, k * k * Ci
    T = {"x": nhwc(x.detach(), ldx, 1), "w": w.detach().permute(0, 2, 3, 1).reshape(Co, K).reshape(-1).clone(),
         "b": bias, "dy": nhwc(dy, ldy, 2)}
    geo = dict(KH=k, KW=k, dil=dil, pad=pad, stride=stride, Ho=Ho, Wo=Wo)
    # forward: rows = output pixels
    M = n * Ho * Wo
    T["C"] = torch.full((M * ldy + 1,), float("nan"), dtype=F64)
    d = R.desc(a_mode=R.A_CONV, M=M, N=Co, K=K, A=R.operand("x", ldx, 1), B=R.operand("w", K), conv=R.conv(H, W, Ci, **geo),
               ldc_m=ldy, bias="b")
    C64, mask = run(d, T)
    same(C64[:M * ldy].view(n, Ho, Wo, ldy)[..., :Co], y.detach().permute(0, 2, 3, 1))
    assert int(mask.sum()) == M * Co
    # weight gradient: A = dy^T (pixels x Co), B = im2col(x)^T
    T["C"] = torch.zeros(Co * K, dtype=F64)
    d = R.desc(a_mode=R.A_MC, b_mode=R.B_CONVW, M=Co, N=K, K=M, A=R.operand("dy", ldy, 2), B=R.operand("x", ldx, 1),
               conv=R.conv(H, W, Ci, **geo))
    C64, _ = run(d, T)
    same(C64.view(Co, k, k, Ci), gw.permute(0, 2, 3, 1))
    # ... and in split-K slabs with a short last one
    ks = 7
    nz = -(-M // ks) + 1
    T["C"] = torch.zeros(nz * Co * K, dtype=F64)
    d = R.desc(a_mode=R.A_MC, b_mode=R.B_CONVW, M=Co, N=K, K=M, batch=nz, ksplit=ks, c_bso=Co * K,
               A=R.operand("dy", ldy, 2), B=R.operand("x", ldx, 1), conv=R.conv(H, W, Ci, **geo))
    C64, _ = run(d, T)
    same(C64.view(nz, Co, k, k, Ci).sum(0), gw.permute(0, 2, 3, 1))
    assert float(C64.view(nz, -1)[-1].abs().max()) == 0.0
    # input gradient (stride 1 only): mirrored taps over dy, weights as [Ci, (tap, Co)]
    if stride == 1 and (Ho, Wo) == (H, W):
        T["wd"] = w.detach().permute(1, 2, 3, 0).reshape(-1).clone()
        T["C"] = torch.zeros(n * H * W * Ci, dtype=F64)
        d = R.desc(a_mode=R.A_CONV, M=n * H * W, N=Ci, K=k * k * Co, A=R.operand("dy", ldy, 2),
                   B=R.operand("wd", k * k * Co), conv=R.conv(H, W, Co, KH=k, KW=k, dil=dil, pad=pad, sign=-1))
        C64, _ = run(d, T)
        same(C64.view(n, H, W, Ci), gx.permute(0, 2, 3, 1))


def test_conv_two_sources_repeat():
    """Channels ci >= C1 come from src2 of image img // rep: torch.cat + repeat_interleave."""
    n2, rep, C1, C2, Co, H, W = 2, 3, 3, 2, 4, 6, 5
    x1, x2 = rnd(n2 * rep, C1, H, W, seed=12), rnd(n2, C2, H, W, seed=13)
    w = rnd(Co, C1 + C2, 3, 3, seed=14)
    y = F.conv2d(torch.cat([x1, x2.repeat_interleave(rep, 0)], 1), w, padding=2, dilation=2)
    K, M = 9 * (C1 + C2), n2 * rep * H * W
    T = {"x1": nhwc(x1, C1 + 2), "x2": nhwc(x2, C2 + 1, 3), "w": w.permute(0, 2, 3, 1).reshape(-1).clone(),
         "C": torch.zeros(M * Co, dtype=F64)}
    d = R.desc(a_mode=R.A_CONV, M=M, N=Co, K=K, A=R.operand("x1", C1 + 2), B=R.operand("w", K),
               conv=R.conv(H, W, C1, KH=3, KW=3, dil=2, pad=2, C2=C2, rep=rep, src2="x2", src2_off=3, ld2=C2 + 1))
    C64, _ = run(d, T)
    same(C64.view(n2 * rep, H, W, Co), y.permute(0, 2, 3, 1))


def test_conv_transpose_2x_store_and_bias_mod():
    n, Ci, Co, H, W = 2, 5, 3, 4, 3
    x, w, b = rnd(n, Ci, H, W, seed=15), rnd(Ci, Co, 2, 2, seed=16), rnd(Co, seed=17)
    y = F.conv_transpose2d(x, w, b, stride=2)
    ldo = Co + 2
    T = {"x": nhwc(x, Ci), "w": w.permute(2, 3, 1, 0).reshape(-1).clone(), "b": b,
         "C": torch.full((n * 4 * H * W * ldo,), float("nan"), dtype=F64)}
    d = R.desc(M=n * H * W, N=4 * Co, K=Ci, A=R.operand("x", Ci), B=R.operand("w", Ci), out_mode=R.OUT_CONVT2X, ldc_m=ldo,
               ct=(H, W, Co), bias="b", bias_mod=Co)
    C64, mask = run(d, T)
    same(C64.view(n, 2 * H, 2 * W, ldo)[..., :Co], y.permute(0, 2, 3, 1))
    assert int(mask.sum()) == n * 4 * H * W * Co and not bool(mask.view(-1, ldo)[:, Co:].any())


# ---------------------------------------------------------------------------------------------------------- patches
@pytest.mark.parametrize("n,C,H,W,P", [(2, 3, 8, 12, 4), (1, 3, 37, 50, 16), (1, 1, 801, 801, 16)])
def test_patch_gather_scatter_and_transposed_twin(n, C, H, W, P):
    img = rnd(n, C, H, W, seed=18)
    npy, npx = -(-H // P), -(-W // P)
    cols = F.unfold(F.pad(img, (0, npx * P - W, 0, npy * P - H)), P, stride=P).transpose(1, 2)   # [n, tokens, C P P]
    tok, K, E = npy * npx, C * P * P, 6
    w, pos, dy = rnd(E, K, seed=19), rnd(tok + 1, E, seed=20), rnd(n * tok, E, seed=21)
    T = {"img": img.reshape(-1), "w": w.reshape(-1), "pos": pos.reshape(-1), "dy": dy.reshape(-1),
         "C": torch.full((n * (tok + 1) * E,), float("nan"), dtype=F64)}
    d = R.desc(a_mode=R.A_PATCH, M=n * tok, N=E, K=K, A=R.operand("img"), B=R.operand("w", K),
               conv=R.conv(H, W, C, patch=P), out_mode=R.OUT_PATCH, ct=(tok, 0, 0), resid="pos")
    C64, mask = run(d, T)
    out = C64.view(n, tok + 1, E)
    same(out[:, 1:], cols @ w.t() + pos[1:])
    assert not bool(mask.view(n, tok + 1, E)[:, 0].any()) and bool(mask.view(n, tok + 1, E)[:, 1:].all())
    assert bool(out[:, 0].isnan().all()), "class-token rows are not addressed"
    # weight gradient of the patch embedding: dW[e, (c, i, j)] = sum over tokens
    T["C"] = torch.zeros(E * K, dtype=F64)
    d = R.desc(a_mode=R.A_MC, b_mode=R.B_PATCHT, M=E, N=K, K=n * tok, A=R.operand("dy", E), B=R.operand("img"),
               conv=R.conv(H, W, C, patch=P))
    C64, _ = run(d, T)
    same(C64.view(E, K), dy.t() @ cols.reshape(n * tok, K))


# ---------------------------------------------------------------------------------------------------------- producers
def test_gelu_and_layernorm_producers():
    Kt, M, N = 13, 4, 7
    dy, x, ga, be = rnd(Kt, M, seed=22), rnd(Kt, N, seed=23) * 2, rnd(N, seed=24), rnd(N, seed=25)
    T = {"dy": padded(dy, M + 1), "x": padded(x, N + 2, 1), "C": torch.zeros(M * N, dtype=F64), "ga": ga, "be": be}
    d = R.desc(a_mode=R.A_MC, b_mode=R.B_NC_GELU, M=M, N=N, K=Kt, A=R.operand("dy", M + 1), B=R.operand("x", N + 2, 1))
    same(run(d, T)[0].view(M, N), dy.t() @ F.gelu(x))
    eps = 1e-5
    mean, var = x.mean(1), x.var(1, unbiased=False)
    T["st"] = torch.stack([mean, (var + eps).rsqrt()], 1).reshape(-1)
    d = R.desc(a_mode=R.A_MC, b_mode=R.B_NC_LN, M=M, N=N, K=Kt, A=R.operand("dy", M + 1), B=R.operand("x", N + 2, 1),
               b_stats="st", b_gamma="ga", b_beta="be")
    same(run(d, T)[0].view(M, N), dy.t() @ F.layer_norm(x, (N,), ga, be, eps))


# ---------------------------------------------------------------------------------------------------------- epilogue
def _epi_case(act, accumulate=False, resid=True, bias_mod=3, preact=False):
    M, N, K = 5, 6, 4
    a, b, bias, r, c0 = rnd(M, K, seed=26), rnd(N, K, seed=27), rnd(N, seed=28), rnd(M, N, seed=29), rnd(M, N, seed=30)
    T = {"A": a.reshape(-1), "B": b.reshape(-1), "bias": bias, "R": padded(r.t().contiguous(), M + 2, 3),
         "C": padded(c0, N + 1, 4), "P": torch.full((7 + M * (N + 1),), float("nan"), dtype=F64)}
    d = R.desc(M=M, N=N, K=K, A=R.operand("A", K), B=R.operand("B", K), c_off=4, ldc_m=N + 1, alpha=-0.37, bias="bias",
               bias_mod=bias_mod, act=act, accumulate=accumulate, preact="P" if preact else None, p_off=7,
               resid="R" if resid else None, r_off=3, ldr_m=1, ldr_n=M + 2)
    res = R.reference_full(d, T)
    v = -0.37 * (a @ b.t()) + (bias[torch.arange(N) % bias_mod] if bias_mod else bias)
    out = res.C64[4:4 + M * (N + 1)].view(M, N + 1)[:, :N]
    return out, v, r, c0, res


def test_epilogue_order_and_bias_mod():
    out, v, r, c0, res = _epi_case(R.ACT_RELU, accumulate=True, preact=True)
    same(out, F.relu(v) + r + c0)       # resid AFTER the activation, bias[n % 3]
    same(res.P64[7:].view(5, 7)[:, :6], v)
    assert int(res.p_mask.sum()) == 30 and not bool(res.p_mask[:7].any())
    out, v, r, c0, _ = _epi_case(R.ACT_GELU, bias_mod=0)
    same(out, F.gelu(v) + r)
    out, v, r, c0, _ = _epi_case(R.ACT_NONE, resid=False, accumulate=True)
    same(out, v + c0)


def test_backward_activations_read_resid_as_z():
    out, v, z, c0, _ = _epi_case(R.ACT_MUL_DGELU)
    zz = z.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(F.gelu(zz), zz, v)
    same(out, g)
    out, v, z, c0, _ = _epi_case(R.ACT_MUL_DRELU, accumulate=True)
    same(out, v * (z > 0) + c0)


def test_column_major_store_and_written_mask():
    """ldc_m = 1, ldc_n = HW (the cosine-classifier store) with an odd offset: the mask is exactly M x N elements."""
    M, N, K, HW = 7, 3, 5, 9
    a, b = rnd(M, K, seed=31), rnd(N, K, seed=32)
    T = {"A": a.reshape(-1), "B": b.reshape(-1), "C": torch.full((3 + N * HW + 2,), float("nan"), dtype=F64)}
    d = R.desc(M=M, N=N, K=K, A=R.operand("A", K), B=R.operand("B", K), c_off=3, ldc_m=1, ldc_n=HW)
    C64, mask = run(d, T)
    same(C64[3:3 + N * HW].view(N, HW)[:, :M], (a @ b.t()).t())
    want = torch.zeros(N, HW, dtype=torch.bool)
    want[:, :M] = True
    assert torch.equal(mask[3:3 + N * HW].view(N, HW), want) and int(mask.sum()) == M * N


# ---------------------------------------------------------------------------------------------------------- the bound
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_GELU, R.ACT_RELU, R.ACT_MUL_DGELU])
def test_bound_holds_for_an_fp32_evaluation_and_is_not_vacuous(act):
    """torch's fp32 CPU kernels are one admissible fp32 evaluation: inside the bound, and the bound stays within 64 x of
    the fp32 result's own size times K u (it is an error bound, not a tolerance)."""
    M, N, K = 40, 30, 300
    a, b, bias, r = (rnd(M, K, seed=33).float(), rnd(N, K, seed=34).float(), rnd(N, seed=35).float(),
                     rnd(M, N, seed=36).float())
    T = {"A": a.reshape(-1), "B": b.reshape(-1), "bias": bias, "R": r.reshape(-1), "C": torch.zeros(M * N)}
    d = R.desc(M=M, N=N, K=K, A=R.operand("A", K), B=R.operand("B", K), alpha=0.5, bias="bias", act=act, resid="R")
    C64, mask, bound = R.reference(d, T)
    v = 0.5 * (a @ b.t()) + bias
    if act == R.ACT_GELU:
        got = F.gelu(v) + r
    elif act == R.ACT_RELU:
        got = F.relu(v) + r
    elif act == R.ACT_MUL_DGELU:
        z = r.clone().requires_grad_(True)
        (got,) = torch.autograd.grad(F.gelu(z), z, v)
    else:
        got = v + r
    err = (got.double().reshape(-1) - C64).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(bound.max()) <= 64 * K * R.U * float(C64.abs().max())


def test_erf_terms_are_twice_the_measured_distance():
    x = torch.cat([torch.linspace(-12, 12, 4_000_001), 2.0 ** -torch.arange(0, 41.0), -(2.0 ** -torch.arange(0, 41.0))]).float()
    x = x[x != 0]
    rel = float(((F.gelu(x).double() - R.gelu64(x.double())).abs() / x.double().abs()).max())
    z = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(F.gelu(z).sum(), z)
    dabs = float((g.double() - R.dgelu64(x.double())).abs().max())
    assert 1.0 * rel <= R.ERF_GELU_REL <= 2.05 * rel, rel
    assert 1.0 * dabs <= R.ERF_DGELU_ABS <= 2.05 * dabs, dabs
    xs = torch.linspace(-6, 6, 1_200_001, dtype=F64)
    assert abs(float(R.dgelu64(xs).abs().max()) - R.GELU_LIPSCHITZ) <= 1e-9
    assert abs(float(R.dgelu64(torch.tensor(math.sqrt(2.0), dtype=F64))) - R.GELU_LIPSCHITZ) <= 1e-9
