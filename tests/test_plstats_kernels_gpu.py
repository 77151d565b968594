"""svl_pl_stats_i64 (and the meter's svl_pl_add_losses) against the int64 restatement tests/plstats_ref.py: exact equality
everywhere -- these are integer counts, there is no tolerance.  Sizes around the wave (64) and the block (256), two trips
of the capped grid plus 5, both load paths (16-byte and scalar), the contention case (one class everywhere), the edges
of every predicate, accumulation, guard bands, bit-equal reruns and the launcher's refusals."""
import numpy as np
import pytest
import torch

import plstats_ref as R

pytestmark = pytest.mark.gpu
GUARD = 16
SENTINEL = -0x0123456789ABCDEF


def make(n, N, seed, dev, coherent=False):
    g = torch.Generator().manual_seed(seed)
    if coherent:        # runs of one class, like a label map's rows
        run = 37
        base = torch.randint(0, N, ((n + run - 1) // run,), generator=g)
        gt = base.repeat_interleave(run)[:n].clone()
    else:
        gt = torch.randint(0, N, (n,), generator=g)
    p = torch.where(torch.rand(n, generator=g) < 0.6, gt, torch.randint(0, N, (n,), generator=g))
    conf = torch.rand(n, generator=g) ** 0.25
    ign = torch.where(torch.rand(n, generator=g) < 0.1, 255, 0)
    mc = torch.where(torch.rand(n, generator=g) < 0.5, torch.where(torch.rand(n, generator=g) < 0.5, gt, p), 255)
    gt = torch.where(torch.rand(n, generator=g) < 0.05, 255, gt)
    gt = torch.where(ign == 255, 254, gt)
    return dict(mask_w=p.to(dev), conf=conf.to(dev), ign=ign.to(dev), mc=mc.to(dev), gt=gt.to(dev))


def run(d, N, bins, thresh, use_mc=True, use_gt=True, stats=None):
    """The kernel on a table between two guard bands -> (table, guards intact)."""
    from semivl_amd import ops
    T = R.table_len(N, bins)
    if stats is None:
        stats = torch.full((GUARD + T + GUARD,), SENTINEL, dtype=torch.int64, device=d["mask_w"].device)
        stats[GUARD:GUARD + T] = 0
    ops.pl_stats(d["mask_w"], d["conf"], d["ign"], stats[GUARD:GUARD + T], N, bins, thresh,
                 mc=d["mc"] if use_mc else None, gt=d["gt"] if use_gt else None)
    return stats


def check(d, N, bins, thresh, use_mc=True, use_gt=True):
    T = R.table_len(N, bins)
    stats = run(d, N, bins, thresh, use_mc, use_gt)
    want = R.pl_stats_ref(d["mask_w"], d["conf"], d["ign"], N, bins, thresh, mc=d["mc"] if use_mc else None,
                          gt=d["gt"] if use_gt else None)
    got = stats[GUARD:GUARD + T]
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, (bad[:8], got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert (stats[:GUARD] == SENTINEL).all() and (stats[GUARD + T:] == SENTINEL).all(), "guard bands"
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("N,bins", [(1, 1), (2, 20), (19, 20), (21, 1), (21, 20), (150, 20)])
def test_small_sizes_match_the_restatement(dev, n, N, bins):
    d = make(n, N, 100 * N + n, dev)
    got = check(d, N, bins, 0.9)
    assert int(got[-1]) == n


@pytest.mark.parametrize("use_mc,use_gt", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("N", [21, 150])
def test_optional_maps_present_and_null(dev, N, use_mc, use_gt):
    d = make(5000, N, 7 + N, dev, coherent=True)
    got = check(d, N, 20, 0.9, use_mc, use_gt)
    rows = got[:13 * N].view(13, N)
    assert rows[0].sum() > 0 and rows[1].sum() > 0
    for r_ in (2, 3):
        assert bool(rows[r_].any()) is use_mc
    for r_ in (4, 5, 6, 7, 8, 9):
        assert bool(rows[r_].any()) is use_gt
    for r_ in (10, 11, 12):
        assert bool(rows[r_].any()) is (use_mc and use_gt)
    assert bool(got[13 * N + 20:13 * N + 40].any()) is use_gt


@pytest.mark.parametrize("coherent", [False, True])
def test_two_trips_of_the_capped_grid_plus_five(dev, coherent):
    from semivl_amd import lib as L
    n = 2 * int(L.load().svl_pl_stats_pass_pixels()) + 5
    assert n == 2 * 2048 * 256 * 2 + 5
    d = make(n, 21, 5, dev, coherent=coherent)
    got = check(d, 21, 20, 0.9)
    assert int(got[-1]) == n and int(got[:21].sum()) == int((d["ign"] != 255).sum())


def test_every_pixel_ignored(dev):
    d = make(777, 21, 3, dev)
    d["ign"].fill_(255)
    got = check(d, 21, 20, 0.5)
    assert not got[:-1].any() and int(got[-1]) == 777


@pytest.mark.parametrize("N,c", [(1, 0), (21, 0), (21, 20), (150, 77)])
def test_every_pixel_the_same_class(dev, N, c):
    """The contention case: all 64 lanes of every wave carry one class in all three maps and one confidence bin."""
    n = 70001
    d = dict(mask_w=torch.full((n,), c, dtype=torch.int64, device=dev), conf=torch.full((n,), 0.97, device=dev),
             ign=torch.zeros(n, dtype=torch.int64, device=dev), mc=torch.full((n,), c, dtype=torch.int64, device=dev),
             gt=torch.full((n,), c, dtype=torch.int64, device=dev))
    got = check(d, N, 20, 0.95)
    rows = got[:13 * N].view(13, N)
    assert (rows[:, c] == n).all() and int(rows.sum()) == 13 * n and int(got[13 * N + 19]) == n


def test_labels_outside_the_classes_count_nowhere(dev):
    N, n = 21, 4099
    d = make(n, N, 11, dev)
    d["mask_w"][::3] = -1
    d["mask_w"][1::5] = 255
    d["mask_w"][2::7] = N
    d["gt"][::4] = 254
    d["gt"][1::9] = 255
    d["gt"][2::11] = -1
    d["gt"][3::13] = N
    d["mc"][::6] = -1
    d["mc"][1::8] = N
    got = check(d, N, 20, 0.9)
    valid = d["ign"] != 255
    inside = (d["mask_w"] >= 0) & (d["mask_w"] < N)
    assert int(got[:N].sum()) == int((valid & inside).sum()) < int(valid.sum())


def test_confidence_edges(dev):
    """conf exactly at thresh (confident), one ulp below (not), exactly 1.0 (last bin), 0.0, -0.0, negative, NaN (bin 0, not
    confident), +inf (last bin, confident)."""
    N, bins = 5, 20
    for thresh in (0.95, 0.5, 0.05):
        t32 = np.float32(thresh)
        vals = [t32, np.nextafter(t32, np.float32(0)), np.nextafter(t32, np.float32(1)), 1.0, 0.0, -0.0, -0.25, float("nan"),
                float("inf"), 0.05, 0.1, 0.15, 0.35, 0.7, 0.999999]
        n = 64 * len(vals) + 3
        d = make(n, N, 23, dev)
        d["ign"].fill_(0)
        d["conf"] = torch.tensor(vals, dtype=torch.float32, device=dev).repeat_interleave(2).repeat(40)[:n].contiguous()
        got = check(d, N, bins, thresh)
        conf = d["conf"].cpu().numpy()
        with np.errstate(invalid="ignore"):
            assert int(got[N:2 * N].sum()) == int((conf >= t32).sum())
        hist = got[13 * N:13 * N + bins]
        assert int(hist.sum()) == n and int(hist[0]) >= int((~(conf > 0)).sum()) and int(hist[bins - 1]) >= int((conf >= 1).sum())


@pytest.mark.parametrize("off_maps,off_conf", [(1, 0), (0, 1), (1, 1), (0, 2)])
@pytest.mark.parametrize("n", [257, 1030])
def test_misaligned_maps_take_the_scalar_path(dev, n, off_maps, off_conf):
    """Maps 8 bytes off a 16-byte boundary and conf 4 bytes off: the scalar loads; (0, 2): conf 8 bytes off still vector."""
    N = 21
    d = make(n + 2, N, 31 + n, dev, coherent=True)
    e = {k: (v[off_conf:off_conf + n] if k == "conf" else v[off_maps:off_maps + n]) for k, v in d.items()}
    assert all(v.is_contiguous() for v in e.values())
    assert e["mask_w"].data_ptr() % 16 == 8 * off_maps and e["conf"].data_ptr() % 16 == 4 * off_conf
    check(e, N, 20, 0.9)
    # only ONE optional map off the boundary
    f = dict(d, mc=d["mc"][1:n + 1], **{k: d[k][:n] for k in ("mask_w", "conf", "ign", "gt")})
    check(f, N, 20, 0.9)


def test_two_calls_accumulate_and_reruns_are_bit_equal(dev):
    N, bins, T = 21, 20, R.table_len(21, 20)
    a, b = make(9001, N, 41, dev, coherent=True), make(6007, N, 42, dev)
    wa = R.pl_stats_ref(a["mask_w"], a["conf"], a["ign"], N, bins, 0.9, mc=a["mc"], gt=a["gt"])
    wb = R.pl_stats_ref(b["mask_w"], b["conf"], b["ign"], N, bins, 0.9, mc=b["mc"])
    s = run(a, N, bins, 0.9)
    s = run(b, N, bins, 0.9, use_gt=False, stats=s)
    assert torch.equal(s[GUARD:GUARD + T], wa + wb)
    assert (s[:GUARD] == SENTINEL).all() and (s[GUARD + T:] == SENTINEL).all()
    s2 = run(b, N, bins, 0.9, use_gt=False, stats=run(a, N, bins, 0.9))
    assert torch.equal(s, s2)


def test_refusals_name_the_function(dev):
    from semivl_amd import lib as L
    from semivl_amd.ops import _p
    lib = L.load()
    d = make(64, 21, 1, dev)
    stats = torch.zeros(R.table_len(21, 20), dtype=torch.int64, device=dev)
    m, c, i, s = _p(d["mask_w"]), _p(d["conf"]), _p(d["ign"]), _p(stats)
    bad = [((m, c, i, None, None, 64, 0, 20, 0.9, s), "N = 0 < 1"), ((m, c, i, None, None, 64, -3, 20, 0.9, s), "N = -3 < 1"),
           ((m, c, i, None, None, 64, 21, 0, 0.9, s), "bins = 0 < 1"), ((m, c, i, None, None, 0, 21, 20, 0.9, s), "n = 0 < 1"),
           ((m, c, i, None, None, 64, 1261, 0 + 1, 0.9, s), "64 KB"), ((m, c, i, None, None, 64, 21, 8056, 0.9, s), "64 KB"),
           ((m, c, i, None, None, 1 << 44, 21, 20, 0.9, s), "2^32"),
           ((None, c, i, None, None, 64, 21, 20, 0.9, s), "null"), ((m, None, i, None, None, 64, 21, 20, 0.9, s), "null"),
           ((m, c, None, None, None, 64, 21, 20, 0.9, s), "null"), ((m, c, i, None, None, 64, 21, 20, 0.9, None), "null")]
    for args, word in bad:
        assert lib.svl_pl_stats_i64(*args, None) == -1, word
        err = L.last_error()
        assert "svl_pl_stats_i64" in err and word in err, err
    torch.cuda.synchronize()
    assert not stats.any()
    # the largest tables that fit are taken: 13 * 1260 + 2 counters = 65528 B; 13 * 21 + 2 * 8055 = 16383 counters
    n = 1000
    big = make(n, 1260, 2, dev)
    check(big, 1260, 1, 0.9)
    check(make(n, 21, 3, dev), 21, 8055, 0.9)
    from semivl_amd import ops
    with pytest.raises(ValueError, match="stats"):
        ops.pl_stats(d["mask_w"], d["conf"], d["ign"], stats[:-1], 21, 20, 0.9)
    with pytest.raises(ValueError, match="conf"):
        ops.pl_stats(d["mask_w"], d["conf"].double(), d["ign"], stats, 21, 20, 0.9)
    with pytest.raises(ValueError, match="gt"):
        ops.pl_stats(d["mask_w"], d["conf"], d["ign"], stats, 21, 20, 0.9, gt=d["gt"][:-1])


def test_meter_update_and_losses(dev):
    """PseudoLabelMeter on the device: update = the kernel, add_losses sums in float64 and counts, report / reset; a changed
    conf_thresh and mismatched maps are refused."""
    from semivl_amd.monitor import PseudoLabelMeter
    N, bins = 21, 20
    meter = PseudoLabelMeter(N, bins, device=dev)
    d = make(2 * 24 * 20, N, 51, dev, coherent=True)
    maps = {k: v.view(2, 24, 20) for k, v in d.items()}
    meter.update(maps["mask_w"], maps["conf"], maps["ign"], 0.9, mclip=maps["mc"], mask_u=maps["gt"])
    meter.update(maps["mask_w"], maps["conf"], maps["ign"], 0.9)
    want = (R.pl_stats_ref(d["mask_w"], d["conf"], d["ign"], N, bins, 0.9, mc=d["mc"], gt=d["gt"])
            + R.pl_stats_ref(d["mask_w"], d["conf"], d["ign"], N, bins, 0.9))
    assert torch.equal(meter.table, want)
    with pytest.raises(ValueError, match="conf_thresh"):
        meter.update(maps["mask_w"], maps["conf"], maps["ign"], 0.95)
    with pytest.raises(ValueError, match="mask_u"):
        meter.update(maps["mask_w"], maps["conf"], maps["ign"], 0.9, mask_u=maps["gt"][:1])
    with pytest.raises(ValueError, match="conf_w"):
        meter.update(maps["mask_w"], maps["conf"].double(), maps["ign"], 0.9)
    with pytest.raises(ValueError, match="mclip"):
        meter.update(maps["mask_w"], maps["conf"], maps["ign"], 0.9, mclip=maps["mc"].int())
    assert torch.equal(meter.table, want), "a refused update adds nothing"
    l1 = torch.tensor([1.0, 0.1, 0.2, 0.3, 0.4, 1e-3, 2e-3, 3e-3], device=dev)
    l2 = torch.tensor([3.0, 0.5, 0.25, 0.125, 1.0, 0.0, 7e-3, 1e-8], device=dev)
    meter.add_losses(l1)
    meter.add_losses(l2)
    rep = meter.report()
    assert rep["steps"] == 2 and np.array_equal(rep["table"], want.cpu().numpy())
    from semivl_amd.train import LOSS_NAMES
    mean = (l1.double() + l2.double()).cpu().numpy() / 2.0
    assert [rep["train/" + n_] for n_ in LOSS_NAMES] == mean.tolist()
    assert 0 < rep["pl_miou"] < 1 and rep["pixels"] == 2 * 960
    with pytest.raises(ValueError, match="fp32"):
        meter.add_losses(l1[:7])
    meter.reset()
    assert not meter.table.any() and not meter.loss_sum.any() and int(meter.steps) == 0
    meter.update(maps["mask_w"], maps["conf"], maps["ign"], 0.95)       # after reset() another threshold is fine
    assert int(meter.report()["pixels"]) == 960
