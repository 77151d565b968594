"""CPU: the restatements of tests/imgnorm_ref.py proved against independent expressions (ATen float64 F.group_norm /
F.batch_norm with running statistics, and their autograd), the derived bounds measured on the very inputs
tests/test_imgnorm_kernels_gpu.py uses (a plain fp32 evaluation of the header's formulas has to stay inside each of them, and no
ReLU mask may be undecided), and the evidence that the bounds would catch a subtly wrong kernel: eight seeded mutations, each
of which has to exceed the bound on at least one case.  -s prints the measured-to-bound ratios."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import imgnorm_ref as R

TIGHT = 1e-9          # float64 restatement against float64 ATen: both are exact up to ~1e-12 times the conditioning (<= 1e4 here)


def _close(a, b, tol=TIGHT):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _ratio(tag, got, want, bound):
    """max |got - want| / bound; where the bound is zero the values have to be equal."""
    err = (got.double() - want).abs()
    z = bound <= 0
    assert bool((err[z] == 0).all()), tag
    r = float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0
    print(f"[{tag}] fp32 error / bound = {r:.3f}")
    assert r <= 1.0, (tag, r)
    return r


def _exceeds(mut, want, bound):
    return bool(((mut.double() - want).abs() > bound).any())


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


# ------------------------------------------------------------------------------------------------ GroupNorm: the restatement
def _gn_aten(x, dy, gamma, beta, G, relu):
    imgs, HW, C = x.shape
    xn = x.double().permute(0, 2, 1).reshape(imgs, C, HW, 1).requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.group_norm(xn, G, ga, be, R.EPS)
    if relu:
        y = F.relu(y)
    gx, gg, gb = torch.autograd.grad(y, (xn, ga, be), dy.double().permute(0, 2, 1).reshape(imgs, C, HW, 1))
    back = lambda t: t.reshape(imgs, C, HW).permute(0, 2, 1)
    return back(y.detach()), back(gx), gg, gb


@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: c[0])
def test_groupnorm_restatement_is_aten_float64(case):
    name, imgs, HW, C, G, relu, variant = case
    x, dy, gamma, beta = R.gn_inputs(case)
    fwd = R.gn_fwd_ref(x, gamma, beta, G, relu)
    bwd = R.gn_bwd_ref(x, dy, fwd, gamma)
    y, gx, gg, gb = _gn_aten(x, dy, gamma, beta, G, relu)
    assert _close(fwd["y"], y) and _close(bwd["dx"], gx) and _close(bwd["dgamma"], gg) and _close(bwd["dbeta"], gb), name
    st = fwd["st"]
    xg = x.double().view(imgs, HW, G, C // G)
    assert _close(st["mean"], xg.mean((1, 3))) and _close(st["rstd"], 1 / torch.sqrt(xg.var((1, 3), unbiased=False) + R.EPS))
    t, _ = R.gn_table_ref(st, gamma, beta)
    assert _close(x.double() * t[:, 0][:, None] + t[:, 1][:, None], fwd["p"])


def test_groupnorm_constant_image_landmarks():
    """A constant image: the variance is exactly 0, rstd = 1 / sqrt(eps), the normalised value exactly 0: y = beta (relu(beta))."""
    for name in ("one_quad_per_group_const", "tail_4pr_plus_1_const"):
        case = R.gn_case(name)
        x, dy, gamma, beta = R.gn_inputs(case)
        fwd = R.gn_fwd_ref(x, gamma, beta, case[4], case[5])
        assert bool((fwd["st"]["var"] == 0).all()) and bool((fwd["st"]["mean"] == R.GN_CONST).all())
        assert bool((fwd["st"]["rstd"] == 1 / np.sqrt(R.EPS)).all())
        want = beta.double().clamp_min(0) if case[5] else beta.double()
        assert torch.equal(fwd["y"], want.expand_as(fwd["y"]))


# ------------------------------------------------------------------------------------------------ GroupNorm: fp32 inside the bound
def _gn_fp32(x, dy, gamma, beta, G, relu):
    """The header's formulas in fp32: double sums rounded to float, the affine form with fused multiply-adds, fp32 group
    sums, one rounding per product and sum of the dx expression."""
    imgs, HW, C = x.shape
    cg = C // G
    n = HW * cg
    xg = x.double().view(imgs, HW, G, cg)
    m64 = xg.sum((1, 3)) / n
    v64 = ((xg * xg).sum((1, 3)) / n - m64 * m64).clamp_min(0)
    mean, rstd = m64.float(), (1 / torch.sqrt(v64 + R.EPS)).float()
    m, r = mean.repeat_interleave(cg, 1), rstd.repeat_interleave(cg, 1)
    sc = r * gamma
    sh = _fma(-m, sc, beta.expand_as(m))
    p = _fma(x, sc[:, None].expand_as(x), sh[:, None].expand_as(x))
    y = p.clamp_min(0) if relu else p
    d = dy * (p > 0) if relu else dy
    xh = (x - m[:, None]) * r[:, None]
    A, B = d.double().sum(1).float(), (d.double() * xh.double()).sum(1).float()
    S1 = (gamma * A).view(imgs, G, cg).sum(2).repeat_interleave(cg, 1)[:, None]
    S2 = (gamma * B).view(imgs, G, cg).sum(2).repeat_interleave(cg, 1)[:, None]
    inv_n = np.float32(1.0) / (np.float32(HW) * np.float32(cg))
    dx = r[:, None] * (d * gamma - float(inv_n) * (S1 + xh * S2))
    return dict(stats=torch.stack((mean, rstd), 2), table=torch.stack((sc, sh), 1), y=y, dx=dx, cs=torch.stack((A, B), 1),
                dbeta=A.sum(0), dgamma=B.sum(0))


@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: c[0])
def test_groupnorm_fp32_stays_inside_the_bound(case):
    name, imgs, HW, C, G, relu, variant = case
    x, dy, gamma, beta = R.gn_inputs(case)
    fwd = R.gn_fwd_ref(x, gamma, beta, G, relu)
    if relu:                    # no ReLU mask is left to chance: the GPU file compares every element
        assert R.undecided(fwd["p"], fwd["dp"]) == 0, name
    bwd = R.gn_bwd_ref(x, dy, fwd, gamma)
    got = _gn_fp32(x, dy, gamma, beta, G, relu)
    _ratio(f"gn stats {name}", got["stats"], *R.gn_stats_pair(fwd["st"]))
    _ratio(f"gn table {name}", got["table"], *R.gn_table_ref(fwd["st"], gamma, beta))
    _ratio(f"gn y {name}", got["y"], fwd["y"], fwd["bound"])
    _ratio(f"gn chan_sums {name}", got["cs"], bwd["cs"], bwd["dcs"])
    _ratio(f"gn dx {name}", got["dx"], bwd["dx"], bwd["ddx"])
    _ratio(f"gn dgamma {name}", got["dgamma"], bwd["dgamma"], bwd["ddgamma"])
    _ratio(f"gn dbeta {name}", got["dbeta"], bwd["dbeta"], bwd["ddbeta"])


def test_groupnorm_switch_cases_share_their_data():
    a, b = R.gn_inputs(R.gn_case("wide_at_switch")), R.gn_inputs(R.gn_case("narrow_below_switch"))
    assert a[0].shape[1] * a[0].shape[2] == R.GN_WIDE and torch.equal(a[0][:, :-1], b[0]) and torch.equal(a[2], b[2])
    c = R.gn_case("apply_second_trip")
    assert c[2] > R.GN_APPLY_CAP * (256 // (c[3] // 4)) * 8


# ------------------------------------------------------------------------------------------------ BatchNorm: the restatement
@pytest.mark.parametrize("case", R.BN_CASES, ids=lambda c: c[0])
def test_batchnorm_restatement_is_aten_float64(case):
    name, rows, C, relu, res, variant, momentum, running = case
    x, dy, gamma, beta, resid, rm, rv = R.bn_inputs(case)
    f = R.bn_fwd_from_x(x, gamma, beta, resid, relu, momentum, rm, rv)
    b = R.bn_bwd_ref(x, dy, f["mask"], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, rows)
    if rows == 1:               # ATen refuses one value per channel in training: the landmarks instead
        assert bool((f["fin"]["var"] == 0).all()) and torch.equal(f["y"], beta.double()[None])
        assert _close(f["fin"]["running_var"][0], (1 - R.f32(momentum)) * rv.double())
        assert torch.equal(b["dx"], torch.zeros_like(b["dx"]))
        return
    xd = x.double().requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rd = resid.double().requires_grad_(True) if res else None
    rm_t, rv_t = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(xd, rm_t, rv_t, ga, be, training=True, momentum=R.f32(momentum), eps=R.EPS)
    y = y + rd if res else y
    y = F.relu(y) if relu else y
    g = torch.autograd.grad(y, [xd, ga, be] + ([rd] if res else []), dy.double())
    tol = 1e-7 if variant == "bigmean" else TIGHT        # var = E x^2 - mean^2 in float64 at mean^2 = 1e4 var
    assert _close(f["y"], y.detach(), tol) and _close(b["dx"], g[0], tol), name
    assert _close(b["sums"][1], g[1], tol) and _close(b["sums"][0], g[2], tol)
    assert _close(f["fin"]["running_mean"][0], rm_t, tol) and _close(f["fin"]["running_var"][0], rv_t, tol)
    if res:
        assert torch.equal(b["dres"], g[3])
    # eval mode on the updated running statistics
    inv, _ = R.bn_eval_invstd_ref(rv_t)
    pe, _, _ = R.bn_pre_ref(x, rm_t, torch.zeros_like(rm_t), inv, torch.zeros_like(inv), gamma, beta)
    assert _close(pe, F.batch_norm(x.double(), rm_t, rv_t, gamma.double(), beta.double(), training=False, eps=R.EPS), tol)


def test_batchnorm_shards_are_one_big_batch():
    """SyncBN: the sums of two shards finalised with count = all rows are the statistics of the whole batch, and each shard's
    dx with the summed backward sums and that count is its rows of the whole batch's dx."""
    case = R.bn_case(R.BN_SHARD[0])
    k, rows = R.BN_SHARD[1], case[1]
    x, dy, gamma, beta, resid, rm, rv = R.bn_inputs(case)
    f = R.bn_fwd_from_x(x, gamma, beta, None, True)
    s = R.bn_stats_ref(x[:k])[0] + R.bn_stats_ref(x[k:])[0]
    assert _close(s, f["sums"], 1e-14)
    whole = R.bn_bwd_ref(x, dy, f["mask"], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, rows)
    part = [R.bn_bwd_ref(x[sl], dy[sl], f["mask"][sl], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, rows)
            for sl in (slice(0, k), slice(k, rows))]
    tot = part[0]["sums"] + part[1]["sums"]
    assert _close(tot, whole["sums"], 1e-13)
    for sl, pt in zip((slice(0, k), slice(k, rows)), part):
        o = R.bn_dx_ref(pt["dres"], pt["xh"], pt["dxh"], tot[0], 0 * tot[0], tot[1], 0 * tot[1], f["fin"]["invstd"][0],
                        f["fin"]["invstd"][1], gamma.double(), rows)
        assert _close(o["dx"], whole["dx"][sl], 1e-13)


# ------------------------------------------------------------------------------------------------ BatchNorm: fp32 inside the bound
def _bn_fp32(x, dy, gamma, beta, resid, relu, momentum, rm, rv, count):
    xd = x.double()
    sums = torch.stack((xd.sum(0), (xd * xd).sum(0)))
    mu = sums[0] / count
    var = (sums[1] / count - mu * mu).clamp_min(0)
    mean, inv = mu.float(), (1 / torch.sqrt(var + R.EPS)).float()
    mom = R.f32(momentum)
    unb = var * count / (count - 1) if count > 1 else var
    nrm, nrv = ((1 - mom) * rm.double() + mom * mu).float(), ((1 - mom) * rv.double() + mom * unb).float()
    q = ((x - mean) * inv) * gamma + beta
    p = q + resid if resid is not None else q
    y = p.clamp_min(0) if relu else p
    d = dy * (p > 0) if relu else dy
    xh = (x - mean) * inv
    s = torch.stack((d.double().sum(0), (d.double() * xh.double()).sum(0)))
    s0, s1 = s[0].float(), s[1].float()
    inv_n = float(np.float32(1.0 / count))
    dx = gamma * inv * (d - inv_n * (s0 + xh * s1))
    return dict(sums=sums, mean=mean, invstd=inv, running_mean=nrm, running_var=nrv, y=y, dres=d, bsums=s, dx=dx)


@pytest.mark.parametrize("case", R.BN_CASES, ids=lambda c: c[0])
def test_batchnorm_fp32_stays_inside_the_bound(case):
    name, rows, C, relu, res, variant, momentum, running = case
    x, dy, gamma, beta, resid, rm, rv = R.bn_inputs(case)
    f = R.bn_fwd_from_x(x, gamma, beta, resid, relu, momentum, rm, rv)
    if relu:
        assert R.undecided(f["p"], f["dp"]) == 0, name
    b = R.bn_bwd_ref(x, dy, f["mask"], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, rows)
    got = _bn_fp32(x, dy, gamma, beta, resid, relu, momentum, rm, rv, rows)
    _ratio(f"bn sums {name}", got["sums"], f["sums"], f["dsums"])
    for k in ("mean", "invstd", "running_mean", "running_var"):
        _ratio(f"bn {k} {name}", got[k], *f["fin"][k])
    _ratio(f"bn y {name}", got["y"], f["y"], f["bound"])
    assert torch.equal(got["dres"].double(), b["dres"]), name
    _ratio(f"bn bwd sums {name}", got["bsums"], b["sums"], b["dsums"])
    _ratio(f"bn dx {name}", got["dx"], b["dx"], b["ddx"])
    if rows > 1:                # the constant channel: variance exactly 0, y exactly beta (before residual / ReLU)
        assert bool(f["fin"]["var"][3] == 0) and bool((f["q"][:, 3] == float(beta[3])).all())
    inv, dinv = R.bn_eval_invstd_ref(rv)
    _ratio(f"bn eval invstd {name}", 1 / torch.sqrt(rv + np.float32(R.EPS)), inv, dinv)
    pe, dpe, _ = R.bn_pre_ref(x, rm.double(), torch.zeros(C, dtype=torch.float64), inv, dinv, gamma, beta)
    _ratio(f"bn eval y {name}", ((x - rm) * (1 / torch.sqrt(rv + np.float32(R.EPS)))) * gamma + beta, pe, dpe)


def test_batchnorm_case_geometry():
    """The cases reach what their comments say (the launch geometry the header and the kernels' comments document)."""
    chunks = lambda rows: min(R.BN_MAX_CHUNKS, (rows + 255) // 256)
    assert chunks(R.bn_case("stage2_some_lanes")[1]) == 30 and chunks(R.bn_case("stage2_loop_and_tail")[1]) == 62
    c = R.bn_case("chunk_cap")
    assert chunks(c[1]) == R.BN_MAX_CHUNKS and -(-c[1] // R.BN_MAX_CHUNKS) > 256
    c = R.bn_case("grid_second_trip")
    assert c[1] * (c[2] // 4) > R.BN_GRID_CAP * 256


# ------------------------------------------------------------------------------------------------ the mutations
def _gn_small():
    return [c for c in R.GN_CASES if c[1] * c[2] * c[3] <= 200000 and c[6] == ""]


def _bn_small():
    return [c for c in R.BN_CASES if c[1] * c[2] <= 200000 and c[5] == "" and c[1] > 1]


def test_mutation_biased_running_var():
    hit = 0
    for case in _bn_small():
        x, dy, gamma, beta, resid, rm, rv = R.bn_inputs(case)
        s, ds = R.bn_stats_ref(x)
        good = R.bn_finalize_ref(s, ds, case[1], R.EPS, case[6], rm, rv)
        bad = R.bn_finalize_ref(s, ds, case[1], R.EPS, case[6], rm, rv, unbiased=False)
        hit += _exceeds(bad["running_var"][0], *good["running_var"])
    assert hit >= 1


def test_mutation_eps_outside_the_square_root():
    hit = 0
    for case in _bn_small():
        rv = R.bn_inputs(case)[6]
        hit += _exceeds(R.bn_eval_invstd_ref(rv, eps_outside=True)[0], *R.bn_eval_invstd_ref(rv))
    for case in _gn_small():    # and in the GroupNorm statistics
        x, dy, gamma, beta = R.gn_inputs(case)
        st = R.gn_stats_ref(x, case[4])
        hit += _exceeds(1 / (torch.sqrt(st["var"]) + R.EPS), st["rstd"], st["drstd"])
    assert hit >= 2


def test_mutation_divisor_hw_instead_of_hw_cg():
    hit = 0
    for case in _gn_small():
        x, dy, gamma, beta = R.gn_inputs(case)
        fwd = R.gn_fwd_ref(x, gamma, beta, case[4], case[5])
        good = R.gn_bwd_ref(x, dy, fwd, gamma)
        hit += _exceeds(R.gn_bwd_ref(x, dy, fwd, gamma, n_div=case[2])["dx"], good["dx"], good["ddx"])
    assert hit >= 1


def test_mutation_neighbouring_group():
    hit_f = hit_b = 0
    for case in [c for c in _gn_small() if c[4] > 1]:
        x, dy, gamma, beta = R.gn_inputs(case)
        fwd = R.gn_fwd_ref(x, gamma, beta, case[4], case[5])
        st2 = {k: (v.roll(1, 1) if torch.is_tensor(v) else v) for k, v in fwd["st"].items()}
        p2, dp2 = R.gn_pre_ref(x, st2, gamma, beta)
        y2 = p2.clamp_min(0) if case[5] else p2
        hit_f += _exceeds(y2, fwd["y"], fwd["bound"])
        good = R.gn_bwd_ref(x, dy, fwd, gamma)
        hit_b += _exceeds(R.gn_bwd_ref(x, dy, fwd, gamma, group_shift=1)["dx"], good["dx"], good["ddx"])
    assert hit_f >= 1 and hit_b >= 1


def test_mutation_relu_mask_before_the_residual():
    hit = 0
    for case in [c for c in R.BN_CASES if c[4]]:
        x, dy, gamma, beta, resid, rm, rv = R.bn_inputs(case)
        f = R.bn_fwd_from_x(x, gamma, beta, resid, True)
        hit += _exceeds(torch.where(f["q"] > 0, f["p"], torch.zeros_like(f["p"])), f["y"], f["bound"])
        b = R.bn_bwd_ref(x, dy, f["mask"], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, case[1])
        hit += not torch.equal(dy.double() * (f["q"] > 0), b["dres"])
    assert hit >= 2


def test_mutation_count_replaced_by_rows():
    case = R.bn_case(R.BN_SHARD[0])
    k, rows = R.BN_SHARD[1], case[1]
    x, dy, gamma, beta, resid, rm, rv = R.bn_inputs(case)
    f = R.bn_fwd_from_x(x, gamma, beta, None, True)
    whole = R.bn_bwd_ref(x, dy, f["mask"], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, rows)
    sl = slice(0, k)
    pt = R.bn_bwd_ref(x[sl], dy[sl], f["mask"][sl], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, rows)
    z = torch.zeros(case[2], dtype=torch.float64)
    bad = R.bn_dx_ref(pt["dres"], pt["xh"], pt["dxh"], whole["sums"][0], z, whole["sums"][1], z, *f["fin"]["invstd"], gamma.double(), k)
    assert _exceeds(bad["dx"], whole["dx"][sl], whole["ddx"][sl])
    # and in the forward: the shard's own row count under the summed statistics
    s, ds = R.bn_stats_ref(x)
    good, wrong = R.bn_finalize_ref(s, ds, rows), R.bn_finalize_ref(s, ds, k)
    assert _exceeds(wrong["mean"][0], *good["mean"]) and _exceeds(wrong["invstd"][0], *good["invstd"])


def test_mutation_dgamma_and_dbeta_swapped():
    hit = 0
    for case in _gn_small():
        x, dy, gamma, beta = R.gn_inputs(case)
        b = R.gn_bwd_ref(x, dy, R.gn_fwd_ref(x, gamma, beta, case[4], case[5]), gamma)
        hit += _exceeds(b["dbeta"], b["dgamma"], b["ddgamma"]) and _exceeds(b["dgamma"], b["dbeta"], b["ddbeta"])
    for case in _bn_small():
        x, dy, gamma, beta, resid, rm, rv = R.bn_inputs(case)
        f = R.bn_fwd_from_x(x, gamma, beta, resid, case[3])
        b = R.bn_bwd_ref(x, dy, f["mask"], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, case[1])
        hit += _exceeds(b["sums"].flip(0), b["sums"], b["dsums"])
    assert hit >= 2


def test_mutation_one_pixel_dropped_from_a_sum():
    hit_g = hit_b = hit_s = 0
    for case in [c for c in _gn_small() if c[2] > 1]:
        x, dy, gamma, beta = R.gn_inputs(case)
        fwd = R.gn_fwd_ref(x, gamma, beta, case[4], case[5])
        good = R.gn_bwd_ref(x, dy, fwd, gamma)
        hit_g += _exceeds(R.gn_bwd_ref(x, dy, fwd, gamma, drop_pixel=True)["cs"], good["cs"], good["dcs"])
        st2 = R.gn_stats_ref(x[:, :-1].contiguous(), case[4])          # the forward statistics without the last pixel
        n1 = (case[2] - 1) / case[2]
        hit_s += _exceeds(st2["mean"] * n1, fwd["st"]["mean"], fwd["st"]["dmean"])
    for case in _bn_small():
        x, dy, gamma, beta, resid, rm, rv = R.bn_inputs(case)
        f = R.bn_fwd_from_x(x, gamma, beta, resid, case[3])
        good = R.bn_bwd_ref(x, dy, f["mask"], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, case[1])
        bad = R.bn_bwd_ref(x, dy, f["mask"], *f["fin"]["mean"], *f["fin"]["invstd"], gamma, case[1], rows_used=case[1] - 1)
        hit_b += _exceeds(bad["sums"], good["sums"], good["dsums"])
        hit_b += _exceeds(R.bn_stats_ref(x[:-1])[0], f["sums"], f["dsums"])
    assert hit_g >= 1 and hit_b >= 2 and hit_s >= 1
