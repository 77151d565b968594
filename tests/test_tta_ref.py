"""CPU: the float64 restatements of tests/tta_ref.py against torch's own float64 F.interpolate / softmax / flip, torch's fp32
composition inside the composed bounds on the very cases tests/test_tta_kernels_gpu.py runs, tta_from_cfg's acceptances and
refusals, and predict_tta_ref against the oracle's single-view restatements."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tta_ref as R
from spatial_ref import area_scale


def _torch_accum(src, base, H, W, kind, align, flip, scale):
    """torch's composition in src's dtype: resize, class scores, un-flip, scale, add."""
    u = F.interpolate(src, size=(H, W), mode="bilinear", align_corners=align)
    if kind == 0:
        s = u.softmax(1)
    else:
        T = u.sum(1, keepdim=True)
        s = torch.where(T == 0, torch.zeros_like(u), u / torch.where(T == 0, torch.ones_like(T), T))
    v = s.flip(3) if flip else s
    v = v * torch.tensor(np.float32(scale), dtype=src.dtype)
    return v if base is None else base + v


def _exact_scales(hw, HW, align):
    """The fp32 scale the restatements (and ATen's fp32 path) use is the quotient torch's float64 path forms in double."""
    return all(area_scale(a, b, align) == ((a - 1) / (b - 1) if align and b > 1 else 0.0 if align else a / b)
               for a, b in zip(hw, HW))


# geometries whose scales are exact in fp32 for align_corners False (first four) and True (last four), besides the shared ones
EXACT_GEOMS = [("x0_75_x1_25", 2, (12, 20), (16, 16)), ("half", 1, (32, 48), (16, 24)), ("x4", 2, (8, 5), (32, 20)),
               ("x3_down", 1, (9, 12), (3, 4)), ("ac_x4", 2, (5, 9), (17, 33)), ("ac_half", 2, (9, 7), (5, 4)),
               ("ac_x0_75", 1, (7, 13), (9, 17)), ("ac_third", 1, (10, 13), (4, 5))]


@pytest.mark.parametrize("kind", (0, 1))
@pytest.mark.parametrize("align", (False, True))
@pytest.mark.parametrize("flip", (False, True))
def test_accum_ref_is_torch_float64(kind, align, flip):
    """1e-12 where the fp32 scale is exact.  Elsewhere torch's float64 path uses the double quotient: its coordinates differ
    from the restatement's by less than s 2^-24 <= coord_delta, which the bound's coordinate term covers."""
    resized_exactly = 0
    for name, B, hw, HW in [g[:4] for g in R.ACCUM_GEOMS] + EXACT_GEOMS:
        src, base = R.accum_inputs(name, B, 19, hw, HW, kind)
        for b in (None, base):
            got, bound = R.accum_ref(src, b, *HW, kind, align, flip, 1.0 / 12.0)
            want = _torch_accum(src.double(), None if b is None else b.double(), *HW, kind, align, flip, 1.0 / 12.0)
            if _exact_scales(hw, HW, align):
                assert (got - want).abs().max().item() < 1e-12, name
                resized_exactly += hw != HW and hw != (1, 1) and HW != (1, 1)
            else:
                assert bool(((got - want).abs() <= bound).all()), name
    assert resized_exactly >= 8


@pytest.mark.parametrize("flip", (False, True))
def test_view_ref_is_torch_float64(flip):
    exact = 0
    for name, lead, hw, ohw in R.VIEW_RESIZES + [(n, l, s, s) for n, l, s in R.VIEW_IDENTITY] + [(g[0], (2, 3), g[2], g[3]) for g in EXACT_GEOMS]:
        img = R.view_input(name, lead, hw)
        got, bound = R.view_ref(img, *ohw, flip)
        want = F.interpolate(img.double(), size=ohw, mode="bilinear", align_corners=False)
        want = want.flip(3) if flip else want
        if _exact_scales(hw, ohw, False):
            assert (got - want).abs().max().item() < 1e-12, name
            exact += 1
        else:
            assert bool(((got - want).abs() <= bound).all()), name
        if ohw == hw:
            assert torch.equal(got.float(), img.flip(-1) if flip else img)
    assert exact >= 6


def _fp32_inside(name, B, N, hw, HW):
    worst = 0.0
    for kind in (0, 1):
        src, base = R.accum_inputs(name, B, N, hw, HW, kind)
        for align in (False, True):
            interp = R.interp_ref(src, *HW, align)
            for flip in (False, True):
                for b in (None, base):
                    for scale in R.SCALES:
                        ref, bound = R.accum_ref(src, b, *HW, kind, align, flip, scale, interp=interp)
                        assert bool(torch.isfinite(bound).all()), (name, N, kind, "the bound claims nothing somewhere")
                        got = _torch_accum(src, b, *HW, kind, align, flip, scale)
                        ratio = ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
                        assert ratio <= 1.0, (name, N, kind, align, flip, scale, ratio)
                        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("geom", R.ACCUM_GEOMS, ids=[g[0] for g in R.ACCUM_GEOMS])
def test_torch_fp32_composition_lies_inside_the_bound(geom):
    name, B, hw, HW, _ = geom
    worst = max(_fp32_inside(name, B, N, hw, HW) for N in R.ACCUM_NS)
    print(f"[{name}] torch fp32 error / bound <= {worst:.3f}")


@pytest.mark.parametrize("name", R.ACCUM_THRESHOLD_GEOMS)
def test_torch_fp32_composition_lies_inside_the_bound_at_the_thresholds(name):
    _, B, hw, HW, _ = next(g for g in R.ACCUM_GEOMS if g[0] == name)
    worst = max(_fp32_inside(name, B, N, hw, HW) for N in R.ACCUM_THRESHOLD_NS)
    print(f"[{name}] torch fp32 error / bound <= {worst:.3f}")


@pytest.mark.parametrize("geom", R.ACCUM_BIG, ids=[g[0] for g in R.ACCUM_BIG])
def test_torch_fp32_composition_lies_inside_the_bound_big(geom):
    name, B, hw, HW, _ = geom
    print(f"[{name}] torch fp32 error / bound <= {_fp32_inside(name, B, 2, hw, HW):.3f}")


def test_special_inputs_inside_the_bound():
    # all-equal logits: scale / N
    src = torch.full((2, 21, 5, 7), 3.25)
    for scale in R.SCALES:
        ref, bound = R.accum_ref(src, None, 9, 11, 0, False, True, scale)
        assert (ref - float(np.float32(scale)) / 21).abs().max().item() < 1e-15
        assert ((_torch_accum(src, None, 9, 11, 0, False, True, scale).double() - ref).abs() <= bound).all()
    # zero totals: s = 0 with bound 0 inside the block, for both conventions and both flips
    src = R.zero_total_input()
    for align in (False, True):
        for flip in (False, True):
            ref, bound = R.accum_ref(src, None, 32, 20, 1, align, flip, 1.0)
            exact = bound[:, 0] == 0
            assert int(exact.sum()) >= 2 * 10 * 6 and bool((ref.sum(1)[exact] == 0).all())
            cols = exact.any(0).any(0).nonzero().flatten()
            assert (int(cols.min()) >= 10) if flip else (int(cols.max()) < 10)      # the block follows the mirror
            got = _torch_accum(src, None, 32, 20, 1, align, flip, 1.0).double()
            assert ((got - ref).abs() <= bound).all()


def test_view_fp32_inside_the_bound():
    for name, lead, hw, ohw in R.VIEW_RESIZES:
        img = R.view_input(name, lead, hw)
        for flip in (False, True):
            ref, bound = R.view_ref(img, *ohw, flip)
            got = F.interpolate(img, size=ohw, mode="bilinear", align_corners=False)
            got = got.flip(3) if flip else got
            assert ((got.double() - ref).abs() <= bound).all(), name


def test_tta_from_cfg():
    from semivl_amd.evaluate import tta_from_cfg
    assert tta_from_cfg({}) is None and tta_from_cfg(dict(eval_tta=None)) is None
    assert tta_from_cfg(dict(eval_tta={})) == dict(ratios=(1.0,), flip=False)
    assert tta_from_cfg(dict(eval_tta=dict(ratios=[0.5, 1, 1.5], flip=True))) == dict(ratios=(0.5, 1.0, 1.5), flip=True)
    assert tta_from_cfg(dict(eval_tta=dict(img_ratios=(0.75, np.float32(1.25))))) == dict(ratios=(0.75, 1.25), flip=False)
    assert tta_from_cfg(dict(eval_tta=dict(flip=True, flip_direction="horizontal"))) == dict(ratios=(1.0,), flip=True)
    assert tta_from_cfg(dict(eval_tta=tta_from_cfg(dict(eval_tta=dict(ratios=[2]))))) == dict(ratios=(2.0,), flip=False)
    for bad in (dict(ratios=[]), dict(ratios=()), dict(ratios=1.0), dict(ratios=[0.0]), dict(ratios=[-1]), dict(ratios=[True]),
                dict(ratios=["1"]), dict(ratios=[1.0], img_ratios=[1.0]), dict(flip=1), dict(flip="yes"), dict(scales=[1.0]),
                dict(ratios=[float("nan")]), [1.0], "ms", 1.0):
        with pytest.raises(ValueError):
            tta_from_cfg(dict(eval_tta=bad))
    with pytest.raises(ValueError, match="scales"):
        tta_from_cfg(dict(eval_tta=dict(scales=[1.0])))
    with pytest.raises(NotImplementedError, match="vertical"):
        tta_from_cfg(dict(eval_tta=dict(flip=True, flip_direction="vertical")))


def test_entry_points_refuse_bad_arguments_without_a_launch():
    import semivl_amd.lib as L
    lib = L.load()
    for args in ((None, 1, 3, 4, 5, None, 8, 10, 0, 0, 0, 1.0, 0, None), (1, 1, 0, 4, 5, 1, 8, 10, 0, 0, 0, 1.0, 0, None),
                 (1, 1, 3, 4, 5, 1, 8, 10, 2, 0, 0, 1.0, 0, None)):
        assert lib.svl_tta_accum_f32(*args) == -1 and "svl_tta_accum_f32" in L.last_error()
    assert lib.svl_tta_view_f32(None, 3, 4, 5, 8, 10, 0, None, None) == -1 and "svl_tta_view_f32" in L.last_error()
    assert lib.svl_tta_view_f32(1, 3, 4, 5, 0, 10, 0, 1, None) == -1 and "svl_tta_view_f32" in L.last_error()


def test_predict_tta_ref_single_view_is_the_oracle():
    from oracle import eval_oracle as E
    K, crop, stride = R.EVAL_K, R.EVAL_CFG["crop_size"], R.EVAL_CFG["stride"]
    img, (H, W) = R.eval_image(), R.EVAL_MASK
    toy = E.ToyModel(K)
    with torch.no_grad():
        singles = dict(
            original=(lambda v: toy(v), toy(img).argmax(1), img.shape[-2:]),
            sliding_window=(lambda v: E.predict_sliding_window(toy, v, crop, K)[1],
                            E.predict_sliding_window(toy, img, crop, K)[0], img.shape[-2:]),
            padded_sliding_window=(lambda v: E.predict_padded_sliding_window(toy, v, crop, stride, K)[1],
                                   E.predict_padded_sliding_window(toy, img, crop, stride, K)[0], img.shape[-2:]),
            zegclip_sliding_window=(lambda v: E.predict_zegclip_sliding_window(toy, v, (H, W), crop, stride, K)[1],
                                    E.predict_zegclip_sliding_window(toy, img, (H, W), crop, stride, K)[0], (H, W)))
        for mode, (single, want, size) in singles.items():
            pred, acc, _ = R.predict_tta_ref(single, img, *size, R.KIND[mode], False, (1.0,), False)
            assert acc.shape[-2:] == tuple(size) and torch.equal(pred, want), mode
            assert (acc.sum(1) - 1).abs().max().item() < 1e-12


def test_flipped_view_unflips_onto_the_unflipped_view():
    """A pixelwise model commutes with the mirror, so each flipped view's un-flipped scores are the unflipped view's.  Sizes
    and ratios with exact fp32 scales (1, 2, 0.5): resize and mirror then commute exactly; a mirrored un-flip would not."""
    from oracle import eval_oracle as E
    toy = E.ToyModel(R.EVAL_K).double()
    img = R.eval_image((2, 3, 40, 48)).double()
    with torch.no_grad():
        for r in (1.0, 0.5, 2.0):
            for align in (False,) if r != 1.0 else (False, True):
                plain = R.accum_ref(toy(R.view_ref(img, int(40 * r + 0.5), int(48 * r + 0.5), False)[0]), None, 40, 48, 0, align, False, 1.0)[0]
                flipped = R.accum_ref(toy(R.view_ref(img, int(40 * r + 0.5), int(48 * r + 0.5), True)[0]), None, 40, 48, 0, align, True, 1.0)[0]
                assert (plain - flipped).abs().max().item() < 1e-12, r
                assert (plain - flipped.flip(3)).abs().max().item() > 1e-3       # the image is not mirror-symmetric
