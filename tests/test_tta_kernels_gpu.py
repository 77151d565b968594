"""GPU: svl_tta_view_f32 and svl_tta_accum_f32 (csrc/tta.hip) through semivl_amd.ops against the float64 restatements of
tests/tta_ref.py under the bounds composed there -- no tolerance is chosen here.  Every case writes into sentinel guard bands
that must come back intact and runs twice for a bit-for-bit comparison; with accumulate = 0 the destination starts as NaN,
which must not reach the result.  -s prints error / bound."""
import pytest
import torch

import tta_ref as R

pytestmark = pytest.mark.gpu


def _ratio(tag, got, want, bound):
    """max |got - want| / bound; where the bound is zero the result has to be equal."""
    assert bool(torch.isfinite(got).all()), tag
    err = (got.double() - want).abs()
    z = bound <= 0
    assert bool((err[z] == 0).all()), tag
    r = float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0
    assert r <= 1.0, (tag, r)
    return r


def _run_accum(tag, src, base, HW, kind, align, flip, scale, guard, dev):
    """ops.tta_accum into two fresh guarded buffers (payload: `base`, or NaN when not accumulating): bit-identical, guards
    intact; returns the [B, N, H, W] result."""
    from semivl_amd import ops
    B, N = src.shape[:2]
    n = B * N * HW[0] * HW[1]
    out = []
    for _ in range(2):
        buf, v = R.guarded(n, device=dev, guard=guard)
        assert (v.data_ptr() % 16 == 0) == (guard == R.AGUARD)
        v.copy_(base.reshape(-1)) if base is not None else v.fill_(float("nan"))
        ops.tta_accum(src, v.view(B, N, *HW), kind, align, flip, scale, base is not None)
        out.append((buf, v))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]), f"{tag}: two runs differ"
    assert R.guard_intact(out[0][0], n, guard=guard), f"{tag}: wrote outside its destination"
    return out[0][1].view(B, N, *HW)


def _sweep(name, B, N, hw, HW, guard, dev):
    worst = 0.0
    for kind in (0, 1):
        src, base = [t.to(dev) for t in R.accum_inputs(name, B, N, hw, HW, kind)]
        for align in (False, True):
            interp = R.interp_ref(src, *HW, align)
            for flip in (False, True):
                for b in (None, base):
                    for scale in R.SCALES:
                        tag = f"{name} N={N} kind={kind} align={int(align)} flip={int(flip)} acc={int(b is not None)} scale={scale:.3f}"
                        got = _run_accum(tag, src, b, HW, kind, align, flip, scale, guard, dev)
                        want, bound = R.accum_ref(src, b, *HW, kind, align, flip, scale, interp=interp)
                        worst = max(worst, _ratio(tag, got, want, bound))
    print(f"[{name} N={N}] max error / bound = {worst:.3f}")


@pytest.mark.parametrize("N", R.ACCUM_NS)
@pytest.mark.parametrize("geom", R.ACCUM_GEOMS, ids=[g[0] for g in R.ACCUM_GEOMS])
def test_tta_accum(dev, geom, N):
    """Both kinds, both flips, both corner conventions, accumulate 0 / 1, scale 1 and 1 / 12 on: identity, x4 up, a reduction, a
    1 x 1 target (W = 1), a 1 x 1 source, odd W, W % 4 != 0, and a W % 4 == 0 destination 4 bytes off a 16-byte boundary."""
    name, B, hw, HW, guard = geom
    _sweep(name, B, N, hw, HW, guard, dev)


@pytest.mark.parametrize("N", R.ACCUM_THRESHOLD_NS)
@pytest.mark.parametrize("name", R.ACCUM_THRESHOLD_GEOMS)
def test_tta_accum_around_the_cache_thresholds(dev, name, N):
    """The class counts at which the kernel changes form (LDS-cached with 16-byte stores, LDS-cached scalar, recomputed)."""
    _, B, hw, HW, guard = next(g for g in R.ACCUM_GEOMS if g[0] == name)
    _sweep(name, B, N, hw, HW, guard, dev)


@pytest.mark.parametrize("geom", R.ACCUM_BIG, ids=[g[0] for g in R.ACCUM_BIG])
def test_tta_accum_grid_stride(dev, geom):
    """N = 2 with more work items than one pass of the capped grid, on the 16-byte and on the scalar path."""
    name, B, hw, HW, guard = geom
    _sweep(name, B, 2, hw, HW, guard, dev)


def test_tta_accum_zero_total_gives_exact_zeros(dev):
    src = R.zero_total_input().to(dev)
    base = torch.rand(2, src.shape[1], 32, 20, generator=torch.Generator().manual_seed(5)).to(dev)
    for align in (False, True):
        for flip in (False, True):
            want, bound = R.accum_ref(src, None, 32, 20, 1, align, flip, 1.0 / 12.0)
            zero = bound == 0
            assert int(zero[:, 0].sum()) >= 2 * 10 * 6
            got = _run_accum("zero_total", src, None, (32, 20), 1, align, flip, 1.0 / 12.0, R.AGUARD, dev)
            assert bool((got[zero] == 0).all())
            finite = torch.isfinite(bound)          # (a total as small as its own error bound claims nothing)
            _ratio("zero_total", got[finite], want[finite], bound[finite])
            acc = _run_accum("zero_total_acc", src, base, (32, 20), 1, align, flip, 1.0 / 12.0, R.AGUARD, dev)
            assert torch.equal(acc[zero], base[zero])


def test_tta_accum_equal_logits_give_scale_over_N(dev):
    for N in (1, 21, 150):
        src = torch.full((2, N, 5, 7), 3.25, device=dev)
        for scale in R.SCALES:
            want, bound = R.accum_ref(src, None, 9, 12, 0, False, True, scale)
            assert (want - float(torch.tensor(scale, dtype=torch.float32)) / N).abs().max().item() < 1e-15
            got = _run_accum(f"equal N={N}", src, None, (9, 12), 0, False, True, scale, R.AGUARD, dev)
            print(f"[equal N={N} scale={scale:.3f}] error / bound = {_ratio('equal', got, want, bound):.3f}")


def _run_view(tag, img, ohw, flip, guard, dev):
    from semivl_amd import ops
    lead = img.shape[:-2]
    n = img[..., 0, 0].numel() * ohw[0] * ohw[1]
    out = []
    for _ in range(2):
        buf, v = R.guarded(n, device=dev, guard=guard)
        ops.tta_view(img, *ohw, flip, out=v.view(*lead, *ohw))
        out.append((buf, v))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]), f"{tag}: two runs differ"
    assert R.guard_intact(out[0][0], n, guard=guard), f"{tag}: wrote outside its destination"
    return out[0][1].view(*lead, *ohw)


@pytest.mark.parametrize("guard", (R.AGUARD, R.GUARD), ids=("aligned", "off4"))
def test_tta_view(dev, guard):
    """Identity: a bit-exact copy (negative zeros and infinities included), with flip a bit-exact mirror; three resizes, both
    flips, inside bilinear_fwd_ref's bound with mirrored columns."""
    for name, lead, hw in R.VIEW_IDENTITY:
        img = R.view_input(name, lead, hw).to(dev)
        img[0, 0, 0, 0], img[0, 0, 0, 1], img[0, 0, 1, 0] = -0.0, float("inf"), float("-inf")
        for flip in (False, True):
            got = _run_view(name, img, hw, flip, guard, dev)
            want = img.flip(-1) if flip else img
            assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)), (name, flip)
    for name, lead, hw, ohw in R.VIEW_RESIZES:
        img = R.view_input(name, lead, hw).to(dev)
        for flip in (False, True):
            got = _run_view(name, img, ohw, flip, guard, dev)
            want, bound = R.view_ref(img, *ohw, flip)
            print(f"[view {name} flip={int(flip)}] error / bound = {_ratio(name, got, want, bound):.3f}")


def test_tta_refusals(dev):
    import semivl_amd.lib as L
    lib = L.load()
    src, dst = torch.zeros(1, 3, 4, 5, device=dev), torch.zeros(1, 3, 8, 10, device=dev)
    p = lambda t: t.data_ptr()
    good = (p(src), 1, 3, 4, 5, p(dst), 8, 10, 0, 0, 0, 1.0, 0, None)
    assert lib.svl_tta_accum_f32(*good) == 0
    for i, v in ((0, None), (5, None), (8, 2), (8, -1), (2, 0), (1, 0), (3, 0), (7, -3)):
        bad = list(good)
        bad[i] = v
        assert lib.svl_tta_accum_f32(*bad) == -1 and "svl_tta_accum_f32" in L.last_error(), i
    good = (p(src), 3, 4, 5, 8, 10, 1, p(dst), None)
    assert lib.svl_tta_view_f32(*good) == 0
    for i, v in ((0, None), (7, None), (1, 0), (2, 0), (5, -1)):
        bad = list(good)
        bad[i] = v
        assert lib.svl_tta_view_f32(*bad) == -1 and "svl_tta_view_f32" in L.last_error(), i
    torch.cuda.synchronize()
