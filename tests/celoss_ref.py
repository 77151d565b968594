"""Float64 restatement of the labelled cross entropy with label smoothing and class weights, i.e. of
nn.CrossEntropyLoss(weight=w, ignore_index=255, label_smoothing=eps) on [B, N, ...] logits (the reference builds its
labelled criterion as nn.CrossEntropyLoss(**cfg['criterion']['kwargs']), semivl.py:142-143).

With t_i the target of pixel i, v_i = [t_i != 255], p = softmax(x_i), lse_i = logsumexp(x_i), W = sum_c w_c (w = ones when
absent) and D = sum_i v_i w_{t_i}:

    num_i = v_i [ (1 - eps) w_{t_i} (lse_i - x_{i,t_i}) + (eps / N) sum_c w_c (lse_i - x_{i,c}) ]
    loss  = sum_i num_i / D
    dloss/dx_{i,c} = g v_i [ (1 - eps) w_{t_i} (p_c - [c = t_i]) + (eps / N) (W p_c - w_c) ],   g = factor / D

tests/test_celoss_ref.py holds these functions to torch's own float64 loss and autograd; the GPU tests use them as the
reference of the kernels.  The resized form evaluates ATen's upsample_bilinear2d as two dense matrices, so that the
gradient at the head's resolution is the same matrices transposed."""
import torch

IGNORE = 255


def _w(weight, N):
    return torch.ones(N, dtype=torch.float64) if weight is None else weight.detach().double().cpu().reshape(N)


def celoss(x, target, eps=0.0, weight=None, factor=1.0, g=None):
    """x [B, N, *] (any float dtype, any device), target [B, *] int64 -> dict of float64 CPU tensors:
    loss (0-dim), num [B, *], D (0-dim), grad [B, N, *] = g * (...) with g = factor / D unless `g` is given."""
    x = x.detach().double().cpu()
    t = target.detach().cpu()
    N = x.shape[1]
    w = _w(weight, N)
    xs = x.movedim(1, -1)                                   # [B, *, N]
    lse = torch.logsumexp(xs, dim=-1)
    p = torch.softmax(xs, dim=-1)
    v = t != IGNORE
    ti = torch.where(v, t, torch.zeros_like(t))
    wt = torch.where(v, w[ti], torch.zeros((), dtype=torch.float64))
    xt = xs.gather(-1, ti.unsqueeze(-1)).squeeze(-1)
    smooth = (w * (lse.unsqueeze(-1) - xs)).sum(-1)
    num = torch.where(v, (1.0 - eps) * wt * (lse - xt) + (eps / N) * smooth, torch.zeros((), dtype=torch.float64))
    D = wt.sum()
    onehot = torch.nn.functional.one_hot(ti, N).double()
    gr = (1.0 - eps) * wt.unsqueeze(-1) * (p - onehot) + (eps / N) * (w.sum() * p - w)
    gr = torch.where(v.unsqueeze(-1), gr, torch.zeros((), dtype=torch.float64))
    scale = (factor / D) if g is None else torch.as_tensor(g, dtype=torch.float64)
    # (D = 0: the loss is 0 / 0 like torch's; no element is multiplied by the infinite scale -- every gradient is 0)
    grad = gr * scale if bool(v.any()) else torch.zeros_like(gr)
    return dict(loss=num.sum() / D, num=num, D=D, grad=grad.movedim(-1, 1).contiguous())


def resize_matrix(n_in, n_out, align_corners):
    """[n_out, n_in] float64: one axis of ATen's upsample_bilinear2d (area_pixel_compute_source_index, clamped taps)."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    if align_corners:
        scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    else:
        scale = n_in / n_out
    for o in range(n_out):
        s = scale * o if align_corners else max(scale * (o + 0.5) - 0.5, 0.0)
        i0 = min(int(s), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = min(max(s - i0, 0.0), 1.0)
        m[o, i0] += 1.0 - l1
        m[o, i1] += l1
    return m


def resize(x, H, W, align_corners):
    """bilinear [B, N, h, w] -> [B, N, H, W] in float64 on the CPU."""
    x = x.detach().double().cpu()
    ry, rx = resize_matrix(x.shape[2], H, align_corners), resize_matrix(x.shape[3], W, align_corners)
    return torch.einsum("Yy,bnyx,Xx->bnYX", ry, x, rx)


def resize_transpose(gfull, h, w, align_corners):
    """The resize's transpose: a gradient on [B, N, H, W] carried to [B, N, h, w]."""
    ry, rx = resize_matrix(h, gfull.shape[2], align_corners), resize_matrix(w, gfull.shape[3], align_corners)
    return torch.einsum("Yy,bnYX,Xx->bnyx", ry, gfull.double().cpu(), rx)


def celoss_up(x, H, W, align_corners, target, eps=0.0, weight=None, factor=1.0, g=None):
    """celoss on resize(x); `grad` is taken to x's own (head) resolution, `grad_full` stays at [H, W]."""
    out = celoss(resize(x, H, W, align_corners), target, eps, weight, factor, g)
    out["grad_full"] = out["grad"]
    out["grad"] = resize_transpose(out["grad_full"], x.shape[2], x.shape[3], align_corners)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs and limits the GPU tests share (tests/test_celoss_kernels_gpu.py; tests/test_celoss_ref.py holds torch's own
# fp32 loss to the same limits on the same inputs)
LOSS_TOL = 1e-5            # |sums[0] / sums[3] - loss|
D_RTOL = 1e-6              # sums[3] against D (exactly the integer count without weights)
GRAD_ATOL_G, GRAD_RTOL = 4e-5, 2e-4     # allclose(dlogits, ref, atol = GRAD_ATOL_G * g, rtol = GRAD_RTOL)

FUSED_SHAPES = [(2, 2, 37), (2, 21, 672), (1, 65, 300), (2, 150, 160), (3, 19, 1031)]          # (B, N, HW)
UP_GEOMS = [(5, 8, 8, 32, 32), (7, 13, 20, 50, 79), (3, 9, 9, 9, 9), (4, 17, 11, 34, 22), (81, 16, 16, 64, 64),
            (150, 24, 40, 96, 160)]                                                             # (N, h, w, H, W)
SETTINGS = ["eps0.1", "weights", "eps0.2_zero_weight", "eps1.0"]


def setting(name, N, seed=7):
    """(eps, weight or None) of one of SETTINGS; weights are fp32 values in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(seed + N)
    w = (torch.rand(N, generator=g) + 0.5).float()
    if name == "eps0.1":
        return 0.1, None
    if name == "weights":
        return 0.0, w
    if name == "eps0.2_zero_weight":
        w[N // 2] = 0.0
        return 0.2, w
    if name == "eps1.0":
        return 1.0, None
    raise KeyError(name)


def logits_and_target(shape_x, shape_t, N, seed):
    """randn x 2 logits; about 10 % of the targets ignored; image 0 carries a fully ignored band: rows 4..11 of a [B, H, W]
    map, the first 32 pixels (at most half) of a flat [B, HW] one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape_x, generator=g) * 2
    t = torch.randint(0, N, shape_t, generator=g)
    t[torch.rand(*shape_t, generator=g) < 0.1] = IGNORE
    if len(shape_t) == 3:
        t[0, 4:12] = IGNORE
    else:
        t[0, :min(32, shape_t[1] // 2)] = IGNORE
    return x, t
