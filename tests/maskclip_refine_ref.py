"""Plain float64 restatement of MaskCLIP's two training-free refinements as ops.mc_refine / MaskClip2Head apply them, written
from the semantics (prompt denoising, key smoothing; F.softmax, torch.max, F.normalize with its default dim = 1), in the
reference's own association (k^ k^^T) P -- none of it from the kernels, which compute k^ (k^^T P) and never form the HW x HW
matrix.  tests/test_maskclip_refine_ref.py holds it at 1e-12 to tests/golden/maskclip_refine.npz (the reference's own code
in float64); the GPU tests hold the kernels to it.

Also here: the error bounds of the stages, each derived from the number formats (U = 2^-24), none from what the kernels give:
  P        tests/rownorm_ref.softmax_fwd_ref with the scale 100 folded in (z = 100 x' rounded once, the maximum, one subtraction,
           expf within an ulp, the sum in any order, one reciprocal, one product);
  s        the squares of fp32 numbers are exact in double and HW of them are added in double, (HW + 4) 2^-53 relative with the
           square root and the quotient, then ONE rounding to fp32: (U + (HW + 4) 2^-53) s;
  product  O = k (s . (k^T P)) from the kernel's own fp32 P and s: no addend passes more than HW roundings in the first
           product, one in the scaling, E in the second; gamma(HW + E + 4) = n U / (1 - n U) times the sum of the magnitudes
           of all addends, |k| (s . (|k|^T |P|)) -- the a-priori bound of an fp32 product in any order of summation;
  end to end from raw inputs: that, plus sum_j |W_ij| (P's bound)_jc, W = k^ k^^T in float64.
"""
import torch

from rownorm_ref import SECOND, U, softmax_fwd_ref

SCALE = 100.0
FILL = -100.0
EPS = 1e-12


def softmax100(x):
    z = SCALE * x
    e = torch.exp(z - z.max(-1, keepdim=True).values)      # a NaN logit: exp(NaN) -> the whole row NaN, as F.softmax gives
    return e / e.sum(-1, keepdim=True)


def nanmax(t, dim):
    """torch.max semantics spelled out: NaN wherever the reduced slice holds one."""
    m = torch.where(torch.isnan(t), torch.full_like(t, -float("inf")), t).max(dim).values
    return torch.where(torch.isnan(t).any(dim), torch.full_like(m, float("nan")), m)


def normalize_dim1(k):
    """F.normalize(k, p=2) on [B, HW, E] with torch's default dim = 1: each channel over the HW tokens of its image."""
    return k / k.pow(2).sum(1, keepdim=True).sqrt().clamp_min(EPS)


def refine_ref(x, k, pd_thresh, ks_thresh):
    """x [B, HW, N], k [B, HW, E] or None (float64) -> dict:
      out [B, N, HW]   what MaskClip2Head hands to the resize (class planes)
      xf [B, HW, N]    the logits after prompt denoising;  peak [B, N] / dropped [B, N] (None / all False without it)
      P, rowmax, selected [B, HW], W [B, HW, HW], O [B, HW, N]   (None unless key smoothing ran)."""
    x = x.double()
    B, HW, N = x.shape
    r = dict(peak=None, dropped=torch.zeros(B, N, dtype=torch.bool), P=None, rowmax=None, selected=None, W=None, O=None)
    xf = x.clone()
    if pd_thresh > 0:
        r["peak"] = nanmax(softmax100(x), 1)
        r["dropped"] = r["peak"] < pd_thresh                  # strict; NaN < t is False: the class is kept
        xf = torch.where(r["dropped"][:, None, :], torch.full_like(x, FILL), x)
    r["xf"], out = xf, xf
    if k is not None and ks_thresh > 0:
        P = softmax100(xf)
        kh = normalize_dim1(k.double())
        W = kh @ kh.transpose(1, 2)
        r["rowmax"] = nanmax(P, 2)
        r["selected"] = r["rowmax"] < ks_thresh
        O = W @ P
        out = torch.where(r["selected"][:, :, None], O, P)
        r.update(P=P, W=W, O=O)
    r["out"] = out.transpose(1, 2).contiguous()
    return r


def keys_ref(x, ln_w, ln_b, eps, in_w, in_b, out_w, out_b):
    """forward_qkv's k for block input x [B, T, E] (float64): out_proj(in_proj_k(ln1 x)), both biases, no residual; the class
    token row removed.  in_w [3E, E] / in_b [3E] hold q | k | v."""
    E = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + eps) * ln_w + ln_b
    kp = y @ in_w[E:2 * E].t() + in_b[E:2 * E]
    return (kp @ out_w.t() + out_b)[:, 1:]


# ------------------------------------------------------------------------------------------------ bounds
def gamma(n):
    return n * U / (1.0 - n * U)


def p_bound(x32, dropped):
    """(P, bound) [B * HW, N] float64 for fp32 logits x32 [B, HW, N]: the softmax-row bound on the filled logits, z = 100 x'.
    A row with a NaN logit is NaN throughout (bound 0: the NaN set is compared on its own)."""
    B, HW, N = x32.shape
    xf = torch.where(dropped[:, None, :], torch.full_like(x32, FILL), x32).reshape(B * HW, N)
    bad = torch.isnan(xf).any(1)
    P, b = softmax_fwd_ref(torch.where(bad[:, None], torch.zeros_like(xf), xf), N, SCALE)
    P[bad], b[bad] = float("nan"), 0.0
    return P, b


def s_ref(k32, B, HW):
    """(s, bound) [B, E] float64 for fp32 keys k32 [B * HW, E]."""
    q = k32.double().view(B, HW, -1).pow(2).sum(1)
    s = 1.0 / q.sqrt().clamp_min(EPS) ** 2
    return s, (U + (HW + 4) * 2.0 ** -53) * s


def product_ref(P32, k32, s32, B, HW):
    """(O, bound) [B * HW, N] float64 from the GIVEN fp32 P, k and s (exact operands)."""
    P, k, s = P32.double().view(B, HW, -1), k32.double().view(B, HW, -1), s32.double().view(B, 1, -1)
    O = k @ (s.transpose(1, 2) * (k.transpose(1, 2) @ P))
    mag = k.abs() @ (s.transpose(1, 2) * (k.abs().transpose(1, 2) @ P.abs()))
    E = k.shape[-1]
    return O.reshape(B * HW, -1), (SECOND * gamma(HW + E + 4) * mag).reshape(B * HW, -1)


# ------------------------------------------------------------------------------------------------ seeded inputs
MARGIN = 1e-3      # every decision of the float64 restatement sits at least this far from its threshold


def draw_case(B, HW, N, E, seed, pd_thresh, ks_thresh, nan_at=None, max_rounds=200):
    """fp32 (x [B, HW, N], k [B, HW, E]): cosines 0.2 + 0.03 N(0, 1) with every third class lowered by 0.12, keys N(0, 1).
    A plain draw leaves some peak or row maximum within 5e-5 of its threshold, where fp32 and float64 may decide differently;
    token rows that cause one are drawn again until every |peak - pd_thresh| and |rowmax - ks_thresh| is >= MARGIN in float64
    (asserted), so that decisions can be compared for equality.  `nan_at` = (b, i, c): that logit is NaN, and the margins are
    those of the case WITH it (its image then keeps every class: the rows' maxima are others than without the NaN)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.zeros(N)
    low[2::3] = 0.12

    def rows(n):
        return (0.2 + 0.03 * torch.randn(n, N, generator=g) - low).float()

    x = rows(B * HW).view(B, HW, N)
    k = torch.randn(B, HW, E, generator=g).float()
    for _ in range(max_rounds):
        if nan_at is not None:
            x[nan_at] = float("nan")
        r = refine_ref(x, k[:, :, :1], pd_thresh, ks_thresh)     # (no decision reads the keys: one channel stands in)
        bad = torch.zeros(B, HW, dtype=torch.bool)
        if r["peak"] is not None:
            near = (r["peak"] - pd_thresh).abs() < MARGIN                       # [B, N]
            at = softmax100(x.double()).argmax(1)                               # the row that holds each class's peak
            for b, c in near.nonzero().tolist():
                bad[b, at[b, c]] = True
        if r["rowmax"] is not None:
            bad |= (r["rowmax"] - ks_thresh).abs() < MARGIN
        if not bool(bad.any()):
            return x, k
        x[bad] = rows(int(bad.sum()))
    raise AssertionError("draw_case: no draw with the margin")


def margins(r, pd_thresh, ks_thresh):
    """(smallest |peak - pd_thresh|, smallest |rowmax - ks_thresh|) over the non-NaN entries (inf when the stage did not run)."""
    def least(t, th):
        if t is None:
            return float("inf")
        d = (t - th).abs()
        d = d[~torch.isnan(d)]
        return float(d.min()) if d.numel() else float("inf")
    return least(r["peak"], pd_thresh), least(r["rowmax"], ks_thresh)
