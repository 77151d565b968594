"""CPU: tests/pixel_loss_ref.py, the float64 reference of tests/test_pixel_loss_kernels_gpu.py, is held to torch's own float64
composition and autograd; torch's fp32 evaluation of the same inputs lies inside every limit the kernels are held to (error /
limit printed, -s); and an fp32 emulation of the kernels' arithmetic with a `fault=` switch shows that each listed mistake
breaks a limit on a case the GPU test runs (the case is named next to the fault) -- the limits are sharp enough to see them."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pixel_loss_ref as R

LOG2E, LN2 = np.float32(1.44269504088896340736), np.float32(0.69314718055994530942)


def _B(N):
    return 1 if N >= 100 else 2


@functools.lru_cache(None)
def fused_inputs(B, N, HW, case):
    return R.case_inputs(case, (B, N, HW), (B, HW), seed=101)


@functools.lru_cache(None)
def up_inputs(geom, case):
    N, h, w, H, W = geom
    return R.case_inputs(case, (_B(N), N, h, w), (_B(N), H, W), seed=102)


# ------------------------------------------------------------------------------------------------ torch's own composition
def torch_ce(x, t, kw, g, dtype, up=None):
    """sums [4] and d(g-weighted loss)/dx by autograd, everything in `dtype` on the CPU (labels inside [0, N) or 255)."""
    x = x.detach().to(dtype).requires_grad_(True)
    full = x if up is None else F.interpolate(x, size=up[:2], mode="bilinear", align_corners=up[2])
    B = x.shape[0]
    t_ok = (t != 255) if kw.get("use_ignore_t", True) else torch.ones_like(t, dtype=torch.bool)
    ce = F.cross_entropy(full, torch.where(t_ok, t, torch.zeros_like(t)), reduction="none")
    w = torch.ones_like(ce)
    valid, sc = t_ok, torch.zeros((), dtype=dtype)
    if kw.get("conf") is not None:
        v = kw["ign"] != 255
        cf = kw["conf"].float()
        w = torch.ones_like(ce) if kw.get("all_pixels") else ((cf >= torch.tensor(kw["conf_thresh"], dtype=torch.float32)) & v).to(dtype)
        if kw.get("img_weight") is not None:
            w = w * kw["img_weight"].to(dtype).view(B, *([1] * (t.dim() - 1)))
        valid, sc = v, (cf.to(dtype) * v).sum()
    s0 = (ce * w * t_ok).sum()
    s1 = torch.zeros((), dtype=dtype)
    if kw.get("mc") is not None:
        s1 = F.cross_entropy(full, kw["mc"], ignore_index=255, reduction="none").sum()
    loss = g[0] * s0 + g[1] * s1
    grad = torch.autograd.grad(loss, x)[0] if loss.requires_grad else torch.zeros_like(x)
    return torch.stack([s0.detach(), s1.detach(), sc.detach() if torch.is_tensor(sc) else sc, valid.sum().to(dtype)]), grad.detach()


def ref_of(x, t, kw, g, up=None):
    if up is None:
        ref = R.ce_plain(x, t, g=g, **kw)
        return ref, R.ce_bounds(ref)
    ref = R.ce_plain_up(x, up[0], up[1], up[2], t, g=g, **kw)
    return ref, R.ce_bounds(ref, (x, *up))


def all_cases():
    """(label, x, t, kw, g, up) of every CE case the GPU test runs."""
    for B, N, HW in R.FUSED_SHAPES:
        for case, form in R.case_forms():
            x, m = fused_inputs(B, N, HW, case)
            t, kw = R.form_kwargs(form, m, B)
            yield f"full B{B} N{N} HW{HW} {case} {form}", x, t, kw, R.form_gscale(form, B * HW), None
    for geom, align in R.up_pairs():
        N, h, w, H, W = geom
        for case, form in R.case_forms():
            x, m = up_inputs(geom, case)
            t, kw = R.form_kwargs(form, m, _B(N))
            yield f"up {geom} align={align} {case} {form}", x, t, kw, R.form_gscale(form, _B(N) * H * W), (H, W, align)


def test_reference_equals_torch_float64_and_its_autograd():
    worst = 0.0
    for label, x, t, kw, g, up in all_cases():
        ref, _ = ref_of(x, t, kw, g, up)
        sums, grad = torch_ce(x, t, kw, g, torch.float64, up)
        scale = ref["sums"].abs().clamp_min(1.0)
        e_s = ((sums - ref["sums"]).abs() / scale).max().item()
        e_g = (grad - ref["grad"]).abs().max().item() / max(g[0] + g[1], 1e-30)
        worst = max(worst, e_s, e_g)
        assert e_s < 1e-12 and e_g < 1e-12, (label, e_s, e_g)
        assert sums[3].item() == ref["sums"][3].item()
    print(f"\nreference against torch float64: largest relative difference {worst:.2e}")


def test_torch_fp32_lies_inside_every_limit():
    worst = {}
    for label, x, t, kw, g, up in all_cases():
        ref, bnd = ref_of(x, t, kw, g, up)
        sums, grad = torch_ce(x, t, kw, g, torch.float32, up)
        r = R.ce_ratios(sums, grad, ref, bnd)
        for k, v in r.items():
            if k == "sum2":        # torch adds conf in its own order and in fp32 throughout: not the kernels' block sums
                continue
            if v > worst.get(k, (0, ""))[0]:
                worst[k] = (v, label)
            assert v <= 1.0, (label, k, v)
    for k, (v, label) in sorted(worst.items()):
        print(f"\ntorch fp32 error / limit, {k}: {v:.4f} at {label}", end="")
    print()


def test_out_of_range_labels_read_no_logit():
    """254, and 255 with use_ignore_t = 0: lse - 0 and g p without a one-hot term, by hand."""
    x, m = fused_inputs(2, 21, 672, "baseline")
    t = m["lab"].clone()
    t[0, ::3] = 254
    t[1, 1::4] = 255
    ref = R.ce_plain(x, t, use_ignore_t=False, g=(0.5, 0.0))
    xd = x.double()
    lse = torch.logsumexp(xd, 1)
    p = torch.softmax(xd, 1)
    bad = t >= 21
    want = torch.where(bad, lse, lse - xd.gather(1, torch.where(bad, torch.zeros_like(t), t).unsqueeze(1))[:, 0])
    assert abs(ref["sums"][0].item() - want.sum().item()) < 1e-9 and ref["sums"][3].item() == t.numel()
    assert torch.allclose(ref["grad"].movedim(1, -1)[bad], 0.5 * p.movedim(1, -1)[bad], rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ softmax-max and labels
def softmax_cases():
    for B, N, HW in R.FUSED_SHAPES:
        for case in R.VALUE_CASES:
            yield f"full B{B} N{N} HW{HW} {case}", fused_inputs(B, N, HW, case)[0], None
    for geom, align in R.up_pairs():
        for case in R.VALUE_CASES:
            yield f"up {geom} align={align} {case}", up_inputs(geom, case)[0], (geom[3], geom[4], align)


def test_softmax_max_reference_torch_and_the_cap_on_excused_pixels():
    worst = 0.0
    for label, x, up in softmax_cases():
        case = label.split()[-1]
        if up is None:
            conf, lab, gap = R.softmax_max(x)
            full64, full32 = x.double(), x
            delta = None
        else:
            conf, lab, gap = R.softmax_max_up(x, *up)
            full64 = F.interpolate(x.double(), size=up[:2], mode="bilinear", align_corners=up[2])
            full32 = F.interpolate(x, size=up[:2], mode="bilinear", align_corners=up[2])
            delta, _ = R.interp_bound(x, *up)
            assert (full64 - R.resize(x, *up)).abs().max().item() <= 1e-12 * max(1.0, x.abs().max().item())
        tc, tl = full64.softmax(1).max(1)
        assert (tc - conf).abs().max().item() < 1e-12      # (float64 roundings of logits near 1000)
        clear = gap > (0 if delta is None else 2 * delta)
        if case in ("equal", "twin"):       # constructed ties have an exact answer: the first index
            first = R.tie_first(case, x.shape[1])
            xe = full64 if up is None else x.double()       # (on the planes themselves: a float64 resize of two equal
            assert bool((R.softmax_max(xe)[1] == first).all()), label    # planes need not be equal to the last bit)
        else:
            assert torch.equal(tl[clear], lab[clear])
            excused = 1.0 - clear.double().mean().item()
            assert excused <= 0.01, (label, excused)
        # torch's fp32 softmax-max inside the limit
        r = R.ratio((full32.softmax(1).amax(1).double() - conf).abs(), R.conf_bound(full64, delta))
        worst = max(worst, r)
        assert r <= 1.0, (label, r)
    print(f"\ntorch fp32 conf error / limit: {worst:.4f}")


def test_maskclip_reference_and_the_cap_on_excused_pixels():
    for name, d, H, W, th, ign in R.maskclip_cases():
        lab, cgap, gap, zb, cb = R.maskclip_labels(d, H, W, 100.0, th, ign)
        up = F.interpolate(d.double(), size=(H, W), mode="bilinear", align_corners=False)
        conf, idx = (100.0 * up).softmax(1).max(1)
        want = torch.where(conf < R.f32(th), torch.full_like(idx, 255), idx)
        if ign is not None:
            want[ign == 255] = 255
        if name in ("N1", "const_tie"):      # exact: conf = 1 resp. 1 / 4 is not below the threshold, the first index wins
            assert bool((lab == 0).all()), name
            continue
        ok = (gap > 2 * zb) & (cgap > cb)
        assert torch.equal(want[ok], lab[ok])
        assert 1.0 - ok.double().mean().item() <= 0.01, name
        if name == "up_1.0":
            assert bool((lab == 255).all())
        if name == "up_image_0.0":
            assert bool((lab[1] == 255).all()) and bool((lab[0][ign[0] != 255] != 255).all())


def test_trivial_restatements():
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(2, 6, 7, generator=g)
    out = R.concept_max(pred, [0, 1, 4, 6], 3)
    assert torch.equal(out[:, 0], pred[:, 0]) and torch.equal(out[:, 1], pred[:, 1:4].max(1).values)
    a, b = torch.randn(2, 3, 5, generator=g), torch.randn(2, 3, 5, generator=g)
    box = torch.tensor([[1.0, 0.999, 2.0, 0.0, 1.0]] * 2)
    o = R.cutmix(a, b, box)
    assert torch.equal(o[:, :, 0], b[:, :, 0]) and torch.equal(o[:, :, 1:4], a[:, :, 1:4]) and torch.equal(o[:, :, 4], b[:, :, 4])
    assert R.count_valid(torch.tensor([0, 255, 254, 255, 3])) == 3


# ------------------------------------------------------------------------------------------------ sharpness
def taps32(n_in, n_out, align, fault):
    """One axis of the kernels' fp32 tap weights (bilinear_index.h) as an [n_out, n_in] fp32 matrix."""
    f = np.float32
    if align:
        scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    else:
        scale = f(n_in) / f(n_out)
    m = np.zeros((n_out, n_in), dtype=np.float32)
    for o in range(n_out):
        s = scale * f(o) if (align or fault == "no_half_pixel") else scale * (f(o) + f(0.5)) - f(0.5)
        raw = s
        if not align and s < 0:
            s = f(0)
        i0 = min(int(s), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = f(raw - f(i0)) if fault == "no_clamp" else f(min(max(s - f(i0), f(0)), f(1)))
        m[o, i0] += f(1) - l1
        m[o, i1] += l1
    return torch.from_numpy(m)


def emulate(x, t, kw, g, up=None, fault=None):
    """fp32 torch emulation of svl_ce_fused_f32 (up = None: two passes, expf) or svl_ce_up_fused_f32 (base 2, p = exp2(x - lse),
    gradient gathered with the fp32 tap weights) -> (sums [4] float64, grad fp32)."""
    x = x.float()
    B, N = x.shape[:2]
    f = torch.float32
    if up is not None:
        H, W, align = up
        ry, rx = taps32(x.shape[2], H, align, fault), taps32(x.shape[3], W, align, fault)
        v = torch.einsum("Yy,bnyx,Xx->bnYX", ry, x * float(LOG2E), rx)
    else:
        v = x
    vs = v.movedim(1, -1)
    m = vs.amax(-1, keepdim=True)
    if fault == "no_max":
        m = torch.zeros_like(m)
    ex = torch.exp2(vs - m) if up is not None else torch.exp(vs - m)
    s = ex.sum(-1, keepdim=True)
    lse = m + (torch.log2(s) if up is not None else torch.log(s))
    p = torch.exp2(vs - lse) if up is not None else ex / s
    lse = lse.squeeze(-1)
    unit = float(LN2) if (up is not None and fault != "no_ln2") else 1.0
    t_ok = (t != 255) if kw.get("use_ignore_t", True) else torch.ones_like(t, dtype=torch.bool)

    def pick(lab):
        inr = (lab >= 0) & (lab < N)
        li = torch.where(inr, lab, torch.zeros_like(lab))
        return torch.where(inr, vs.gather(-1, li.unsqueeze(-1)).squeeze(-1), torch.zeros((), dtype=f)), \
            F.one_hot(li, N).to(f) * inr.unsqueeze(-1)
    w = torch.ones_like(lse)
    valid, sc = t_ok, torch.zeros_like(lse)
    if kw.get("conf") is not None:
        vmask = kw["ign"] != 255
        cf = kw["conf"].float()
        th = torch.tensor(kw["conf_thresh"], dtype=f)
        hit = (cf > th) if fault == "gt_strict" else (cf >= th)
        w = torch.ones_like(lse) if kw.get("all_pixels") else (hit & vmask).to(f)
        if kw.get("img_weight") is not None and fault != "no_img_weight":
            w = w * kw["img_weight"].float().view(B, *([1] * (t.dim() - 1)))
        valid = vmask
        sc = cf if fault == "ign_in_conf" else torch.where(vmask, cf, torch.zeros((), dtype=f))
    xt, oht = pick(t)
    ce_t = torch.where(t_ok, w * (unit * (lse - xt)), torch.zeros((), dtype=f))
    if kw.get("mc") is not None:
        m_ok = kw["mc"] != 255
        xm, ohm = pick(kw["mc"])
        ce_m = torch.where(m_ok, unit * (lse - xm), torch.zeros((), dtype=f))
    else:
        m_ok, ohm, ce_m = torch.zeros_like(t_ok), torch.zeros_like(oht), torch.zeros_like(lse)
    gt = torch.where(t_ok, np.float32(g[0]) * w, torch.zeros((), dtype=f))
    gm = torch.where(m_ok | (fault == "gm_everywhere"), torch.full_like(lse, float(np.float32(g[1]))), torch.zeros((), dtype=f))
    grad = ((gt + gm).unsqueeze(-1) * p - gt.unsqueeze(-1) * oht - gm.unsqueeze(-1) * ohm).movedim(-1, 1)
    if up is not None:
        grad = torch.einsum("Yy,bnYX,Xx->bnyx", ry, grad, rx)
    if fault == "scale_grad":
        grad = grad * np.float32(1 + 2.0 ** -16)
    sums = torch.stack([ce_t.double().sum(), ce_m.double().sum(), sc.double().sum(), valid.sum().double()])
    if fault == "scale_loss":
        sums[0] = sums[0] * (1 + 2.0 ** -16)
    return sums, grad


def emulate_softmax_max(x, up=None, fault=None):
    """The online softmax-max in class order: (conf fp32, label)."""
    x = x.float()
    if up is not None:
        x = torch.einsum("Yy,bnyx,Xx->bnYX", taps32(x.shape[2], up[0], up[2], fault), x, taps32(x.shape[3], up[1], up[2], fault))
    m = torch.full_like(x[:, 0], -math.inf)
    s = torch.zeros_like(m)
    idx = torch.zeros_like(m, dtype=torch.int64)
    for c in range(x.shape[1]):
        xc = x[:, c]
        new = (xc >= m) if fault == "last_max" else (xc > m)
        s = torch.where(new, s * torch.exp(m - xc).nan_to_num(0.0) + 1, s + torch.exp(xc - m))
        idx = torch.where(new, torch.full_like(idx, c), idx)
        m = torch.where(new, xc, m)
    return 1 / s, idx


def _case(kind, key, case, form):
    """The inputs of one named case of the GPU test."""
    if kind == "full":
        B, N, HW = key
        x, m = fused_inputs(B, N, HW, case)
        n, up = B * HW, None
    else:
        geom, align = key
        N, h, w, H, W = geom
        B = _B(N)
        x, m = up_inputs(geom, case)
        n, up = B * H * W, (H, W, align)
    t, kw = R.form_kwargs(form, m, B)
    return x, t, kw, R.form_gscale(form, n), up


BASE_FULL = ("full", (2, 21, 672))
BASE_UP = ("up", ((5, 8, 8, 32, 32), False))
# fault -> the case of the GPU test that sees it, and the figures of ce_ratios that may break
FAULTS = {
    "gt_strict": (BASE_FULL, "baseline", "pixelwise0.7", ("sum0", "grad")),
    "ign_in_conf": (BASE_FULL, "baseline", "pixelwise0.7", ("sum2",)),
    "gm_everywhere": (BASE_FULL, "baseline", "guided", ("grad", "rowsum")),
    "no_img_weight": (BASE_FULL, "baseline", "all_pixels", ("sum0", "grad")),
    "no_max": (BASE_FULL, "plus1000", "supervised", ("sum0", "grad")),
    "scale_grad": (BASE_FULL, "baseline", "supervised", ("grad",)),
    "scale_loss": (BASE_FULL, "baseline", "supervised", ("sum0",)),
    "no_half_pixel": (BASE_UP, "baseline", "supervised", ("sum0", "grad")),
    "no_clamp": (BASE_UP, "baseline", "supervised", ("sum0", "grad")),
    "no_ln2": (BASE_UP, "baseline", "guided", ("sum0", "sum1")),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_each_fault_breaks_a_limit_on_a_case_the_gpu_test_runs(fault):
    (kind, key), case, form, figures = FAULTS[fault]
    assert (case, form) in R.case_forms() and (key in R.FUSED_SHAPES if kind == "full" else key in R.up_pairs())
    if fault in ("scale_grad", "scale_loss"):
        assert case == "baseline" and key[1] <= 21         # the tightness condition of the limits
    x, t, kw, g, up = _case(kind, key, case, form)
    ref, bnd = ref_of(x, t, kw, g, up)
    good = R.ce_ratios(*emulate(x, t, kw, g, up), ref, bnd)
    bad = R.ce_ratios(*emulate(x, t, kw, g, up, fault=fault), ref, bnd)
    print(f"\n{fault}: error / limit without the fault {max(good.values()):.3f}, with it " +
          ", ".join(f"{k} {bad[k]:.3g}" for k in figures))
    assert max(good.values()) <= 1.0, good
    assert max(bad[k] for k in figures) > 1.0, bad


def test_the_emulation_lies_inside_the_limits_everywhere():
    worst = 0.0
    for label, x, t, kw, g, up in all_cases():
        ref, bnd = ref_of(x, t, kw, g, up)
        r = R.ce_ratios(*emulate(x, t, kw, g, up), ref, bnd)
        worst = max(worst, max(r.values()))
        assert max(r.values()) <= 1.0, (label, r)
    print(f"\nfp32 emulation error / limit: {worst:.4f}")


def test_softmax_max_faults():
    """Last maximum wins ties: seen on the two bit-identical planes (full resolution (2, 21, 672), 'twin': no pixel is
    excused there).  The half-pixel offset and the clamp: seen by conf and the labels of (5, 8, 8, 32, 32), 'baseline'."""
    x = fused_inputs(2, 21, 672, "twin")[0]
    _, lab, _ = R.softmax_max(x)
    assert torch.equal(emulate_softmax_max(x)[1], lab)
    assert not torch.equal(emulate_softmax_max(x, fault="last_max")[1], lab)
    geom, up = (5, 8, 8, 32, 32), (32, 32, False)
    x = up_inputs(geom, "baseline")[0]
    conf, lab, gap = R.softmax_max_up(x, *up)
    delta, _ = R.interp_bound(x, *up)
    bound = R.conf_bound(R.resize(x, *up), delta)
    clear = gap > 2 * delta
    c, l = emulate_softmax_max(x, up)
    assert R.ratio((c.double() - conf).abs(), bound) <= 1.0 and torch.equal(l[clear], lab[clear])
    for fault in ("no_half_pixel", "no_clamp"):
        c, l = emulate_softmax_max(x, up, fault=fault)
        assert R.ratio((c.double() - conf).abs(), bound) > 1.0 and not torch.equal(l[clear], lab[clear]), fault
