"""Plain restatements (torch float64 / int64, Python floats) of the small kernels behind the training step's loss assembly
and the evaluator: svl_copy2d_f32, svl_permute4_f32, svl_reduce_slabs_f32, svl_affine_planes_f32, svl_softmax_planes_f32,
svl_iou_hist_i64, svl_conf_ratio_f32, svl_conf_avg_factor, svl_semivl_gscale, svl_semivl_loss, svl_eltwise_f32 -- each from
the header's formula (include/semivl_hip.h) or the reference lines it names, none from the kernels.  Device-agnostic: the
GPU tests (tests/test_small_kernels_gpu.py) run them on the device with ATen as the checker, tests/test_small_kernel_ref.py
proves them on the CPU against independent expressions.  Also here: the DERIVED error bounds of the three kernels that are
not bit-exact, and the seeded inputs both test files share (so the CPU file can show that a plain fp32 evaluation stays
inside the bounds on the very inputs the GPU file uses).

Sizes: GRID_CAP blocks of 256 threads is what `grid_for` (csrc/norm.hip, csrc/pixel_loss.hip) launches at most; a case whose
element count exceeds one_pass(per_thread) makes every thread take a second trip through its grid-stride loop."""
import math

import numpy as np
import torch

U = 2.0 ** -24                 # unit roundoff of fp32 (round to nearest)
GRID_CAP = 256 * 16
SENTINEL = 7.0                 # guard-band value (tests/test_ops_gpu.py::test_dilated_conv3x3_whole_image_tiles)
GUARD = 61                     # guard elements on each side of a written buffer: odd, so the payload is not 16 B aligned


def one_pass(per_thread=1):
    """Elements one pass of the capped grid covers when the launch is sized with grid_for(n, per_thread)."""
    return GRID_CAP * 256 * per_thread


def guarded(n, dtype=torch.float32, device="cpu", fill=SENTINEL, guard=GUARD):
    """(buffer, payload view): n elements with `guard` sentinel elements on each side."""
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device=device)
    return buf, buf[guard:guard + n]


def guard_intact(buf, n, fill=SENTINEL, guard=GUARD):
    ref = torch.full((guard,), fill, dtype=buf.dtype, device=buf.device)
    return torch.equal(buf[:guard], ref) and torch.equal(buf[guard + n:], ref)


# ------------------------------------------------------------------------------------------------ copy2d
def copy2d_indices(off, grp, go, ld, rows, C, device="cpu"):
    """Flat int64 element indices [rows * C] of  off + (i / grp) * go + (i % grp) * ld + c  (the header's formula)."""
    i = torch.arange(rows, dtype=torch.int64, device=device)
    base = off + torch.div(i, grp, rounding_mode="floor") * go + (i % grp) * ld
    return (base[:, None] + torch.arange(C, dtype=torch.int64, device=device)[None, :]).reshape(-1)


def copy2d_ref(src, s_off, sgrp, src_go, src_ld, dst, d_off, dgrp, dst_go, dst_ld, rows, C, accumulate=False):
    """The result buffer (a copy of the flat `dst`, same dtype) after svl_copy2d_f32.  Destination rows are distinct by the
    entry point's contract, so index_put_ without accumulation of duplicates is the whole semantics.  On float64 copies of
    fp32 data the sum dst + src is exact (|exponent difference| < 29 on the tests' data), so `.float()` of the result is the
    correctly rounded fp32 sum."""
    si = copy2d_indices(s_off, sgrp, src_go, src_ld, rows, C, src.device)
    di = copy2d_indices(d_off, dgrp, dst_go, dst_ld, rows, C, src.device)
    assert int(si.min()) >= 0 and int(si.max()) < src.numel() and int(di.min()) >= 0 and int(di.max()) < dst.numel()
    v = src.reshape(-1).index_select(0, si).to(dst.dtype)
    out = dst.reshape(-1).clone()
    if accumulate:
        v = out.index_select(0, di) + v
    out.index_put_((di,), v)
    return out


def copy2d_forms(B=2, T=1025, E=768, img=(2, 3, 600, 700), nclass=21, crop=512):
    """The thirteen call forms of svl_copy2d_f32 in semivl_amd/model/vit.py and semivl_amd/evaluate.py, as
    (name, src shape, dst shape, dst initial value (None = random: the form accumulates or leaves rows untouched), descriptor
    (s_off, sgrp, src_go, src_ld, d_off, dgrp, dst_go, dst_ld, rows, C), accumulate, expr) where expr(src, dst) -> the
    expected dst from the slicing / cat / broadcast expression the call stands for."""
    NP = T - 1
    b, c, h, w = img
    y1, x1 = 88, 189                                   # an odd column offset
    ch, cw = crop, w - x1                              # 512 x 511 window (odd width)

    def f_qkv_v(s, d):      # vit.py:207  dqkv[:, 2E:3E] += dvproj
        d = d.clone()
        d[:, 2 * E:] += s
        return d

    def f_cls_scatter(s, d):  # vit.py:492  x[b * T] = cls_row
        d = d.clone()
        d.view(B, T, E)[:, 0] = s
        return d

    def f_tok_slice(s, d):  # vit.py:513,521,680  v.view(B, T, E)[:, 1:]
        return s.view(B, T, E)[:, 1:].reshape(B * NP, E).clone()

    def f_cls_gather(s, d):  # vit.py:535  xn.view(B, T, E)[:, 0]
        return s.view(B, T, E)[:, 0].clone()

    def f_tok_scatter(s, d):  # vit.py:617,630  cat(zero cls row, tokens)
        return torch.cat((d.view(B, T, E)[:, :1], s.view(B, NP, E)), 1).reshape(B * T, E)

    def f_pos_first(s, d):  # vit.py:686 (accumulate = acc of the sink): dst (+)= dxpre[0:T]
        return s.view(B, T, E)[0].clone()

    def f_pos_first_acc(s, d):
        return d + s.view(B, T, E)[0]

    def f_pos_next(s, d):  # vit.py:688: dst += dxpre[b T : (b + 1) T], b = 1
        return d + s.view(B, T, E)[1]

    def f_crop(s, d):  # evaluate.py:21  img[:, :, y1:y2, x1:x2]
        return s[:, :, y1:y1 + ch, x1:x1 + cw].clone()

    def f_window_add(s, d):  # evaluate.py:29  canvas[:, :, y1:y1+ch, x1:x1+cw] += win
        d = d.clone()
        d[:, :, y1:y1 + ch, x1:x1 + cw] += s
        return d

    ph, pw = h - 512, w - 512                          # evaluate.py:83: the bottom-right window of the padded mode, 88 x 188

    def f_pad(s, d):  # padded[:, :, :ch, :cw] = img[:, :, row:, col:]
        d = d.clone()
        d[:, :, :ph, :pw] = s[:, :, 512:, 512:]
        return d

    tok = (E, NP, T * E, E, 0, NP, NP * E, E, B * NP, E)
    sct = (0, NP, NP * E, E, E, NP, T * E, E, B * NP, E)
    return [
        ("vit207_qkv_v_add", (B * T, E), (B * T, 3 * E), None, (0, B * T, 0, E, 2 * E, B * T, 0, 3 * E, B * T, E), True, f_qkv_v),
        ("vit492_cls_scatter", (E,), (B * T, E), None, (0, 1, 0, 0, 0, 1, T * E, 0, B, E), False, f_cls_scatter),
        ("vit513_feat_tokens", (B * T, E), (B * NP, E), SENTINEL, tok, False, f_tok_slice),
        ("vit521_proj_tokens", (B * T, E), (B * NP, E), SENTINEL, tok, False, f_tok_slice),
        ("vit535_cls_gather", (B * T, E), (B, E), SENTINEL, (0, 1, T * E, 0, 0, 1, E, 0, B, E), False, f_cls_gather),
        ("vit617_dtok_scatter", (B * NP, E), (B * T, E), 0.0, sct, False, f_tok_scatter),
        ("vit630_dfeat_scatter", (B * NP, E), (B * T, E), 0.0, sct, False, f_tok_scatter),
        ("vit680_dtok_slice", (B * T, E), (B * NP, E), SENTINEL, tok, False, f_tok_slice),
        ("vit686_pos_first", (B * T, E), (T, E), SENTINEL, (0, B * T, 0, E, 0, T, 0, E, T, E), False, f_pos_first),
        ("vit686_pos_first_acc", (B * T, E), (T, E), None, (0, B * T, 0, E, 0, T, 0, E, T, E), True, f_pos_first_acc),
        ("vit688_pos_next", (B * T, E), (T, E), None, (T * E, T, 0, E, 0, T, 0, E, T, E), True, f_pos_next),
        ("eval21_crop", img, (b, c, ch, cw), SENTINEL,
         (y1 * w + x1, ch, h * w, w, 0, ch, ch * cw, cw, b * c * ch, cw), False, f_crop),
        ("eval29_window_add", (b, nclass, ch, cw), (b, nclass, h, w), None,
         (0, ch, ch * cw, cw, y1 * w + x1, ch, h * w, w, b * nclass * ch, cw), True, f_window_add),
        ("eval83_pad_window", img, (b, c, crop, crop), 0.0,
         (512 * w + 512, ph, h * w, w, 0, ph, crop * crop, crop, b * c * ph, pw), False, f_pad),
    ]


def copy2d_generic_cases():
    """Descriptors outside the call sites: broadcast sources (src_ld = 0 and src_go = 0), C in {1, 3, 5, 768}, odd element
    offsets on both sides.  (name, src numel, dst numel, descriptor, accumulate)."""
    out = []
    for C in (1, 3, 5, 768):
        rows = 37
        # one source row broadcast to every destination row (src_go = src_ld = 0), destination rows 2 C + 1 apart
        out.append((f"bcast_row_C{C}", C + 9, 7 + rows * (2 * C + 1), (3, 1, 0, 0, 5, 1, 2 * C + 1, 0, rows, C), False))
        # groups of 5 rows: every group re-reads the same 5 source rows (src_go = 0), strided destination
        out.append((f"bcast_group_C{C}", 11 + 5 * (C + 2), 3 + 8 * 5 * (C + 3),
                    (11, 5, 0, C + 2, 3, 5, 5 * (C + 3), C + 3, 40, C), True))
        # every row of a group reads one row (src_ld = 0), groups advance: the batch broadcast of a per-image row
        out.append((f"bcast_in_group_C{C}", 1 + 6 * C, 9 + 6 * 7 * C, (1, 7, C, 0, 9, 7, 7 * C, C, 42, C), True))
    return out


# ------------------------------------------------------------------------------------------------ permute4
CONV_SHAPES = [(128, 128, 3, 3), (64, 160, 3, 3), (128, 640, 1, 1), (128, 1, 7, 7), (1, 32, 3, 3)]
CONVT_SHAPES = [(128, 64), (64, 48)]


def permute4_ref(src, shape, strides):
    return torch.as_strided(src, shape, strides).contiguous()


def conv_pack_tuples(Co, Ci, kh, kw):
    """(shape, strides) of ops.pack_conv_w's two packs and of ops.unpack_conv_wgrad, with the permute each stands for."""
    cs = (Ci * kh * kw, kh * kw, kw, 1)
    return dict(
        fwd=((Co, kh, kw, Ci), (cs[0], cs[2], cs[3], cs[1]), lambda w: w.permute(0, 2, 3, 1)),
        dgrad=((Ci, kh, kw, Co), (cs[1], cs[2], cs[3], cs[0]), lambda w: w.permute(1, 2, 3, 0)),
        unpack=((Co, Ci, kh, kw), (kh * kw * Ci, 1, kw * Ci, Ci), lambda p: p.view(Co, kh, kw, Ci).permute(0, 3, 1, 2)))


def convt_pack_tuples(Cin, Cu):
    """The three ConvTranspose2d(k 2, s 2) permutes of semivl_amd/model/vlg_head.py (weight [Cin, Cu, 2, 2])."""
    return dict(
        fwd=((2, 2, Cu, Cin), (2, 1, 4, 4 * Cu), lambda w: w.permute(2, 3, 1, 0)),                      # n = (a, b, co)
        wgrad=((Cin, Cu, 2, 2), (4 * Cu, 1, 2 * Cu, Cu), lambda p: p.view(Cin, 2, 2, Cu).permute(0, 3, 1, 2)),
        bwd=((Cin, 2, 2, Cu), (4 * Cu, 2, 1, 4), lambda w: w.permute(0, 2, 3, 1)))


# ------------------------------------------------------------------------------------------------ reduce_slabs
def reduce_slabs_ref(out, slabs, accumulate):
    """Slabs added in index order in double, starting from `out` when accumulating, one rounding at the end."""
    s = out.double().reshape(-1).clone() if accumulate else torch.zeros(out.numel(), dtype=torch.float64, device=slabs.device)
    for k in range(slabs.shape[0]):
        s = s + slabs[k].reshape(-1).double()
    return s.float().view(out.shape)


def cancellation_slabs(n, count, device="cpu"):
    """slab 0 = 2^25, slabs 1 .. n-2 = 1, slab n-1 = -2^25: the exact sum is n - 2; an fp32 chain absorbs every 1 (the
    spacing of fp32 at 2^25 is 4) and ends at 0."""
    s = torch.ones(n, count, device=device)
    s[0] = 2.0 ** 25
    s[n - 1] = -2.0 ** 25
    return s


# ------------------------------------------------------------------------------------------------ affine_planes
CLIP_K4 = [[0.229, 0.224, 0.225], [0.485, 0.456, 0.406], [0.48145466, 0.4578275, 0.40821073],
           [0.26862954, 0.26130258, 0.27577711]]      # rows (ls, lm, cm, cs) of semivl_amd/model/builder.py


def affine_cases():
    """(name, x [B, C, H, W] fp32, k4 [4, C] fp32).  The last case exceeds one pass of the grid (per_thread = 4)."""
    g = torch.Generator().manual_seed(4101)
    k5 = torch.randn(4, 5, generator=g)
    k5[3] = k5[3].sign() * (0.2 + k5[3].abs())          # divisors away from zero, both signs, all four rows distinct per channel
    k3 = torch.randn(4, 3, generator=g)
    k3[3] = k3[3].sign() * (0.2 + k3[3].abs())
    return [("clip_C3_odd", torch.randn(2, 3, 37, 41, generator=g) * 2, torch.tensor(CLIP_K4)),
            ("rand_C5_odd", torch.randn(3, 5, 33, 29, generator=g) * 3, k5),
            ("rand_C3_1px", torch.randn(4, 3, 1, 1, generator=g), k3),
            ("clip_C3_801", torch.randn(3, 3, 801, 801, generator=g) * 2, torch.tensor(CLIP_K4))]


def affine_ref(x, k4):
    k = k4.double()[:, None, :, None, None]
    return ((x.double() * k[0] + k[1]) - k[2]) / k[3]


def affine_bound(x, k4):
    """Three fp32 roundings (product or fused multiply-add, subtraction) and one correctly rounded division:
    |y - y64| <= 4 u (|x k0| + |k1| + |k2|) / |k3|, whether or not the compiler contracts the multiply-add."""
    k = k4.double()[:, None, :, None, None]
    return 4 * U * ((x.double() * k[0]).abs() + k[1].abs() + k[2].abs()) / k[3].abs()


# ------------------------------------------------------------------------------------------------ softmax_planes
def softmax_cases():
    """(name, logits [B, N, H, W] fp32).  N in {1, 19, 21, 150}; spreads up to +-200; all-equal logits; odd HW; the last case
    has more than one_pass(1) pixels."""
    g = torch.Generator().manual_seed(4202)
    eq = torch.full((2, 21, 5, 7), 3.25)
    wide = (torch.rand(2, 150, 13, 11, generator=g) * 2 - 1) * 200
    return [("N1", torch.randn(2, 1, 9, 7, generator=g) * 50),
            ("N19_odd", torch.randn(3, 19, 31, 33, generator=g) * 4),
            ("N21_equal", eq),
            ("N21_gain150", torch.randn(2, 21, 25, 27, generator=g) * 150 / 4),
            ("N150_pm200", wide),
            ("N19_grid_stride", torch.randn(1, 19, 1025, 1027, generator=g) * 6)]


def softmax_ref(x):
    return x.double().softmax(dim=1)


def softmax_bound(x):
    """|p - p64| <= 2 (|x_c - max| + N + 5) u p64 + 2^-126: one rounding of the subtraction carried through the exponential
    (relative |x_c - max| u), expf within 1 ulp, an N-term fp32 sum, a reciprocal, a product; 2 x margin; the absolute term
    covers results below the normal range."""
    xd = x.double()
    N = x.shape[1]
    d = (xd - xd.max(dim=1, keepdim=True).values).abs()
    return 2 * (d + N + 5) * U * softmax_ref(x) + 2.0 ** -126


def softmax_sum_bound(N):
    return (N + 4) * U


# ------------------------------------------------------------------------------------------------ iou_hist
def iou_hist_ref(pred, target, K, ignore_index=255):
    """int64 [3K] = (intersection, prediction area, target area) of intersectionAndUnion (third_party/unimatch/util/
    utils.py:91-103): the prediction is set to ignore_index where the target is; each histogram has the K bins [0, K) and
    drops everything outside (np.histogram / torch.histc with bins 0 .. K)."""
    pred, target = pred.reshape(-1).long(), target.reshape(-1).long()
    out = torch.where(target == ignore_index, torch.full_like(pred, ignore_index), pred)

    def hist(v):
        v = v[(v >= 0) & (v < K)]
        return torch.bincount(v, minlength=K)[:K]
    return torch.cat((hist(out[out == target]), hist(out), hist(target)))


# ------------------------------------------------------------------------------------------------ conf_ratio / conf_avg
def conf_ratio_ref(conf, ign, thresh):
    """fp32(#confident valid) / fp32(#valid) per image from integer sums (train_utils.py:39-40: torch's int / int)."""
    B = conf.shape[0]
    valid = (ign != 255).reshape(B, -1)
    t = torch.tensor(thresh, dtype=torch.float32, device=conf.device)
    hi = ((conf.reshape(B, -1) >= t) & valid).sum(1)
    return hi.float() / valid.sum(1).float()


def conf_avg_factor_ref(conf, ign):
    """sum over images of mean over valid pixels of conf, in float64 (train_utils.py:43-46)."""
    B = conf.shape[0]
    valid = (ign != 255).reshape(B, -1)
    return float(((conf.reshape(B, -1).double() * valid).sum(1) / valid.sum(1).double()).sum())


# ------------------------------------------------------------------------------------------------ loss assembly
def gscale_ref(counts, numel_u, lam, factors=None, mc_counts=None):
    """float64 [4][2] = {g_t, g_m} of the branches {x, s1, s2, fp}: the factor each per-pixel CE term carries in
    d(loss)/d(logits) of  loss = (l_x + l_s1 / 4 + l_s2 / 4 + l_fp / 2) / 2 + lam (mc_s1 / 4 + mc_s2 / 4 + mc_fp / 2)
    (semivl.py:267-323) with l_x = S / counts[0], l_u = S f / counts[i], mc = S / n."""
    f = [1.0, 1.0, 1.0] if factors is None else [float(v) for v in factors]
    n = [float(numel_u)] * 3 if mc_counts is None else [float(v) for v in mc_counts]
    c = [float(v) for v in counts]
    lam = float(np.float32(lam))
    wt, wm = (0.25 / 2, 0.25 / 2, 0.5 / 2), (0.25, 0.25, 0.5)
    g = [[(1.0 / 2) / c[0], 0.0]]
    for i in range(3):
        g.append([wt[i] * f[i] / c[i + 1], wm[i] * lam / n[i]])
    return np.array(g, np.float64)


def loss_ref(sums, numel_u, lam, factors=None, mc_counts=None):
    """(out float64 [8], abs float64 [8]): {loss, loss_x, loss_s1, loss_s2, loss_fp, mc_s1, mc_s2, mc_fp} from sums [4][4] =
    per branch {sum w ce_t, sum ce_m, sum conf valid, #valid}, and the sum of the absolute values of each output's terms."""
    f = [1.0, 1.0, 1.0] if factors is None else [float(v) for v in factors]
    n = [float(numel_u)] * 3 if mc_counts is None else [float(v) for v in mc_counts]
    s = [[float(v) for v in row] for row in sums]
    lam = float(np.float32(lam))
    lx = s[0][0] / s[0][3]
    lu = [s[i + 1][0] * f[i] / s[i + 1][3] for i in range(3)]
    mc = [s[i + 1][1] / n[i] for i in range(3)]
    terms = [lx / 2, lu[0] * 0.25 / 2, lu[1] * 0.25 / 2, lu[2] * 0.5 / 2, mc[0] * 0.25 * lam, mc[1] * 0.25 * lam,
             mc[2] * 0.5 * lam]
    out = [math.fsum(terms), lx] + lu + mc
    return np.array(out, np.float64), np.array([math.fsum(abs(t) for t in terms)] + [abs(v) for v in out[1:]], np.float64)


def loss_cases():
    """(name, counts int64[4], sums float64[4][4], numel_u, lam, factors or None, mc_counts or None): all four combinations of
    factors x mc_counts, pixel counts up to 16 * 801^2, lam = 0, and one size whose counts all lie ABOVE 2^24 and are odd
    (32 * 801^2 pixels: not representable in fp32, so a float conversion of a count shows)."""
    rng = np.random.RandomState(4303)
    out = []
    for name, numel, lam in (("small", 2 * 24 * 20, 0.07), ("crop512", 16 * 512 * 512, 0.1), ("crop801", 16 * 801 * 801, 0.05),
                             ("crop801_lam0", 16 * 801 * 801, 0.0), ("above_2p24", 32 * 801 * 801, 0.05)):
        for fac in (False, True):
            for mcc in (False, True):
                counts = np.array([numel - rng.randint(0, numel // 3 + 1) for _ in range(4)], np.int64)
                if name == "above_2p24":
                    counts = np.array([numel - rng.randint(0, numel // 8) for _ in range(4)], np.int64) | 1
                sums = np.zeros((4, 4), np.float64)
                sums[:, 0] = counts * rng.uniform(0.2, 3.0, 4)
                sums[:, 1] = counts * rng.uniform(0.2, 3.0, 4)
                sums[:, 2] = counts * rng.uniform(0.3, 0.99, 4)
                sums[:, 3] = counts
                factors = rng.uniform(0.5, 16.0, 3) if fac else None
                mc_counts = np.array([max(1, int(c * rng.uniform(0.1, 1.0))) for c in counts[1:]], np.int64) if mcc else None
                out.append((f"{name}_f{int(fac)}_m{int(mcc)}", counts, sums, float(numel), lam, factors, mc_counts))
    return out


# ------------------------------------------------------------------------------------------------ eltwise
def gelu_ref(x):
    xd = x.double()
    return 0.5 * xd * (1.0 + torch.erf(xd / math.sqrt(2.0)))


# ------------------------------------------------------------------------------------------------ predict edge geometries
EDGE_CFG = dict(nclass=5, crop_size=64, stride=40)
EDGE_SIZES = [(50, 70), (64, 64), (65, 129), (40, 40)]
EDGE_MODES = [("zeg", "zegclip_sliding_window", 40), ("sw", "sliding_window", 40), ("pd40", "padded_sliding_window", 40),
              ("pd05", "padded_sliding_window", 0.5)]
EDGE_CENTER = (100, 90)
EDGE_GAP_CLIP = 1e-3           # the fixture keeps min(top-2 gap, this): only near-ties matter, and the constant compresses


def edge_cases():
    """(key, mode, cfg, (h, w), mask (H, W)) of tests/golden/eval_edges.npz.  The zegclip mask size differs from the image, so
    the final align-corners resize runs."""
    out = []
    for h, w in EDGE_SIZES:
        for tag, mode, stride in EDGE_MODES:
            mask_hw = (h + 7, w + 5) if tag == "zeg" else (h, w)
            out.append((f"{tag}/{h}x{w}", mode, dict(EDGE_CFG, stride=stride), (h, w), mask_hw))
    out.append((f"cc/{EDGE_CENTER[0]}x{EDGE_CENTER[1]}", "center_crop", dict(EDGE_CFG), EDGE_CENTER, EDGE_CENTER))
    return out


def edge_image(h, w, seed=91):
    g = torch.Generator().manual_seed(seed + 1000 * h + w)
    img = torch.randn(2, 3, h, w, generator=g)
    return torch.nn.functional.avg_pool2d(img, 5, stride=1, padding=2)
