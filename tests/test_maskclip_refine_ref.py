"""CPU: the float64 restatement of MaskCLIP's refinements and keys (tests/maskclip_refine_ref.py) held at 1e-12 to the
reference's own code in float64 (tests/golden/maskclip_refine.npz, written by tests/golden/gen_golden_maskclip.py), and the
fixture's own conditions re-checked from its data."""
import os

import numpy as np
import pytest
import torch

import maskclip_refine_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-12


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(HERE, "golden", "maskclip_refine.npz"), allow_pickle=False)


def _cases(z):
    return sorted({k.split("/")[1] for k in z.files if k.startswith("refine/")})


def _case(z, name):
    x, k = torch.from_numpy(z[f"refine/{name}/x"]), torch.from_numpy(z[f"refine/{name}/k"])
    pd, ks = (float(v) for v in z[f"refine/{name}/thresh"])
    return x, k, pd, ks, torch.from_numpy(z[f"refine/{name}/out"])


def test_fixture_holds_the_cases_the_tests_rely_on(z):
    assert set(_cases(z)) == {"both", "pd_only", "ks_only", "off", "drop_all", "nan", "wide"}
    assert os.path.getsize(os.path.join(HERE, "golden", "maskclip_refine.npz")) < 500_000
    assert float(z["refine/drop_all/thresh"][0]) == 1.5
    assert int(np.isnan(z["refine/nan/x"]).sum()) == 1


@pytest.mark.parametrize("name", ["both", "pd_only", "ks_only", "off", "drop_all", "nan", "wide"])
def test_restatement_matches_the_reference(z, name):
    x, k, pd, ks, want = _case(z, name)
    r = R.refine_ref(x, k, pd, ks)
    assert torch.equal(torch.isnan(r["out"]), torch.isnan(want))
    d = float((r["out"] - want).abs().nan_to_num(0.0).max())
    print(f"{name}: |restatement - reference| {d:.2e}")
    assert d <= TOL
    m = R.margins(r, pd, ks)
    assert min(m) >= R.MARGIN, m
    if name == "off":
        assert torch.equal(r["out"], x.double().transpose(1, 2))                 # both thresholds 0: the logits themselves
    if name == "pd_only":
        dropped = r["dropped"][:, :, None].expand_as(r["out"])
        assert bool((r["out"][dropped] == -100.0).all()) and torch.equal(r["out"][~dropped], x.double().transpose(1, 2)[~dropped])
    if name == "drop_all":
        assert bool(r["dropped"].all()) and bool(r["selected"].all())
    if name in ("both", "ks_only", "wide"):
        f = float(r["selected"].double().mean())
        assert 0.1 <= f <= 0.9
    if name in ("both", "pd_only", "wide"):
        n = r["dropped"].sum(1)
        assert bool((n >= 1).all()) and bool((r["dropped"].shape[1] - n >= 2).all())


def test_nan_case_keeps_classes_and_rows_as_torch_does(z):
    x, k, pd, ks, want = _case(z, "nan")
    r = R.refine_ref(x, k, pd, ks)
    assert bool(torch.isnan(r["peak"][0]).all()) and not bool(r["dropped"][0].any())    # NaN < pd is False: image 0 keeps every class
    assert bool(torch.isnan(r["rowmax"][0, 3])) and not bool(r["selected"][0, 3])
    assert not bool(torch.isnan(want[1]).any())


def test_dim1_rule_is_not_the_per_token_norm(z):
    """F.normalize's default dim on [B, HW, E] is the TOKEN axis; the per-token normalisation would give another map."""
    x, k, pd, ks, want = _case(z, "both")
    kh = R.normalize_dim1(k.double())
    assert float((kh.pow(2).sum(1) - 1.0).abs().max()) < 1e-12                   # unit columns over the tokens of an image
    r = R.refine_ref(x, torch.nn.functional.normalize(k.double(), dim=2) * 1.0, pd, ks)
    assert float((r["out"] - want).abs().max()) > 1e-3


def test_keys_restatement(z):
    g = {n: torch.from_numpy(z["keys/" + n]) for n in ("x", "ln_w", "ln_b", "in_w", "in_b", "out_w", "out_b", "k")}
    k = R.keys_ref(g["x"], g["ln_w"], g["ln_b"], float(z["keys/eps"]), g["in_w"], g["in_b"], g["out_w"], g["out_b"])
    assert k.shape == g["k"].shape and float((k - g["k"]).abs().max()) <= TOL


def test_model_maps_are_the_restatement_of_the_stored_logits_and_keys(z):
    logits, keys = torch.from_numpy(z["model/logits"]), torch.from_numpy(z["model/keys"])
    B, N, hp, wp = logits.shape
    x = logits.reshape(B, N, hp * wp).transpose(1, 2)
    for pd, ks in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.7), (0.5, 0.7)):
        r = R.refine_ref(x, keys if ks > 0 else None, pd, ks)
        want = torch.from_numpy(z[f"model/{pd}_{ks}/map"])
        assert float((r["out"].reshape(B, N, hp, wp) - want).abs().max()) <= TOL
        assert min(R.margins(r, pd, ks)) >= R.MARGIN


def test_bounds_cover_torch_fp32(z):
    """The stage bounds against an fp32 evaluation on the host (ATen): P, s and the product from fp32 P and s."""
    x, k, pd, ks, _ = _case(z, "wide")
    B, HW, N = x.shape
    r = R.refine_ref(x, k, pd, ks)
    P64, pb = R.p_bound(x, r["dropped"])
    xf = torch.where(r["dropped"][:, None, :], torch.full_like(x, R.FILL), x)
    P32 = torch.softmax(100.0 * xf, -1).reshape(B * HW, N)
    assert float((P64 - r["P"].reshape(B * HW, N)).abs().max()) <= TOL
    assert bool(((P32.double() - P64).abs() <= pb).all())
    k2 = k.reshape(B * HW, -1)
    s64, sb = R.s_ref(k2, B, HW)
    s32 = (1.0 / k2.double().view(B, HW, -1).pow(2).sum(1)).float()
    assert bool(((s32.double() - s64).abs() <= sb).all())
    O64, ob = R.product_ref(P32, k2, s32, B, HW)
    kb = k2.view(B, HW, -1)
    O32 = kb @ (s32[:, :, None] * (kb.transpose(1, 2) @ P32.view(B, HW, N)))
    assert bool(((O32.reshape(B * HW, N).double() - O64).abs() <= ob).all())
