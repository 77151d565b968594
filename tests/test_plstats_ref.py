"""CPU: the int64 restatement of svl_pl_stats_i64's table (tests/plstats_ref.py) against the fixture recorded from the
reference's own intersectionAndUnion (tests/golden/plstats_cases.npz), `mask_ratio` against semivl.py:280-281's expression,
PseudoLabelMeter.report's derived values on a CPU-filled table, and the cfg validator."""
import os
import warnings

import numpy as np
import pytest
import torch

import plstats_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plstats_cases.npz")


def load_cases():
    z = np.load(GOLD)
    out = {}
    for name in z["names"].tolist():
        t = lambda k: torch.from_numpy(z[f"{name}/{k}"]) if f"{name}/{k}" in z.files else None
        N, bins = z[f"{name}/cfg"].tolist()
        out[name] = dict(N=N, bins=bins, thresh=float(z[f"{name}/thresh"]), mask_w=t("mask_w"), conf=t("conf"), ign=t("ign"),
                         mc=t("mc"), gt=t("gt"), iut={k: z[f"{name}/{k}_iut"] for k in ("pl", "plc", "mc")})
    return out


CASES = load_cases()


def _table(c):
    return R.pl_stats_ref(c["mask_w"], c["conf"], c["ign"], c["N"], c["bins"], c["thresh"], mc=c["mc"], gt=c["gt"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference_triples(name):
    c = CASES[name]
    assert tuple(c["mask_w"].shape) == (2, 24, 20) and c["N"] in (1, 2, 21)
    tab = _table(c)
    assert tab.dtype == torch.int64 and tab.numel() == R.table_len(c["N"], c["bins"]) and int(tab[-1]) == 2 * 24 * 20
    for tag, (inter, area, target) in zip(("pl", "plc", "mc"), R.triples(tab, c["N"])):
        want = c["iut"][tag]
        assert np.array_equal(inter.numpy(), want[0]), (name, tag)
        assert np.array_equal((area + target - inter).numpy(), want[1]), (name, tag)
        assert np.array_equal(target.numpy(), want[2]), (name, tag)
    assert c["iut"]["pl"][0].sum() > 0 and (c["mc"] is None) == (c["iut"]["mc"][2].sum() == 0)
    if c["mc"] is None:
        N = c["N"]
        assert not tab[2 * N:4 * N].any() and not tab[10 * N:13 * N].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_mask_ratio_is_the_references_conf_ratio(name):
    """semivl.py:280-281: ((conf >= conf_thresh) & (ignore_mask != 255)).sum().item() / (ignore_mask != 255).sum().item()"""
    from semivl_amd.monitor import report_from_table
    c = CASES[name]
    labels = c["mask_w"].clamp(0, c["N"] - 1)       # (rows 0 / 1 count pixels whose label is a class: every pixel of a real step)
    tab = R.pl_stats_ref(labels, c["conf"], c["ign"], c["N"], c["bins"], c["thresh"])
    conf_ratio = ((c["conf"] >= c["thresh"]) & (c["ign"] != 255)).sum().item() / (c["ign"] != 255).sum().item()
    rep = report_from_table(tab.numpy(), c["N"], c["bins"])
    assert rep["mask_ratio"] == conf_ratio and 0 < conf_ratio < 1
    # the histogram's edges are not the threshold's: its total is the same denominator
    assert int(rep["conf_hist"].sum()) == (c["ign"] != 255).sum().item()


def test_report_on_a_cpu_filled_table():
    from semivl_amd.monitor import PseudoLabelMeter
    from semivl_amd.train import LOSS_NAMES
    c = CASES["voc_edges"]
    N, bins = c["N"], c["bins"]
    meter = PseudoLabelMeter(N, bins, device="cpu")
    assert meter.table.numel() == R.table_len(N, bins) and meter.loss_sum.dtype == torch.float64
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        empty = meter.report()
    assert np.isnan(empty["mask_ratio"]) and np.isnan(empty["guidance_agreement"]) and np.isnan(empty["train/loss"])
    assert "pl_miou" not in empty and empty["steps"] == 0 and np.isnan(empty["pl_class_freq"]).all()
    tab = _table(c)
    meter.table.copy_(tab * 3)          # three identical batches
    meter.loss_sum.copy_(torch.arange(8, dtype=torch.float64) * 1.5)
    meter.steps.fill_(3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rep = meter.report()
    r = [tab[i * N:(i + 1) * N].double().numpy() for i in range(13)]
    assert rep["steps"] == 3 and rep["pixels"] == 3 * 960 and np.array_equal(rep["table"], (tab * 3).numpy())
    assert rep["mask_ratio"] == r[1].sum() / r[0].sum()
    assert rep["guidance_coverage"] == r[2].sum() / r[0].sum()
    assert rep["guidance_agreement"] == r[3].sum() / r[2].sum()
    assert np.array_equal(rep["pl_class_freq"], r[0] / r[0].sum())
    assert np.array_equal(rep["guidance_class_freq"], r[2] / r[2].sum())
    assert np.array_equal(rep["conf_hist"], 3 * tab[13 * N:13 * N + bins].numpy())
    for i, name in enumerate(LOSS_NAMES):
        assert rep["train/" + name] == i * 0.5
    for key, (a, b, t) in (("pl", (5, 6, 4)), ("confident_pl", (8, 9, 7)), ("guidance", (11, 12, 10))):
        union = r[b] + r[t] - r[a]
        seen = union != 0
        assert seen.any()
        assert np.array_equal(rep[key + "_iou"][seen], r[a][seen] / union[seen]) and np.isnan(rep[key + "_iou"][~seen]).all()
        assert rep[key + "_miou"] == (r[a][seen] / union[seen]).mean()
        # the reference's own triples give the same IoU
        want = c["iut"]["pl" if key == "pl" else "plc" if key == "confident_pl" else "mc"].astype(np.float64)
        assert np.array_equal(rep[key + "_iou"][seen], want[0][seen] / want[1][seen])
    hist = tab[13 * N:13 * N + bins].double().numpy()
    ok = tab[13 * N + bins:13 * N + 2 * bins].double().numpy()
    assert np.array_equal(rep["pl_acc_per_bin"][hist > 0], ok[hist > 0] / hist[hist > 0]) and (ok <= hist).all()
    for v_ in rep.values():
        assert isinstance(v_, (int, float, np.ndarray)), type(v_)
    meter.reset()
    assert not meter.table.any() and not meter.loss_sum.any() and int(meter.steps) == 0 and meter.conf_thresh is None


def test_report_without_annotations_has_no_iou_keys():
    from semivl_amd.monitor import report_from_table
    c = CASES["voc"]
    tab = R.pl_stats_ref(c["mask_w"], c["conf"], c["ign"], c["N"], c["bins"], c["thresh"], mc=c["mc"])
    rep = report_from_table(tab.numpy(), c["N"], c["bins"])
    assert not {"pl_iou", "pl_miou", "confident_pl_iou", "guidance_miou", "pl_acc_per_bin"} & set(rep)
    assert 0 < rep["guidance_coverage"] < 1 and 0 < rep["guidance_agreement"] < 1


def test_conf_bin_edges():
    conf = torch.tensor([0.0, 0.049999, 0.05, 0.999999, 1.0, 1.5, float("inf"), -0.1, -0.0, float("nan")])
    assert R.conf_bin(conf, 20).tolist() == [0, 0, 1, 19, 19, 19, 19, 0, 0, 0]
    assert R.conf_bin(conf, 1).tolist() == [0] * 10


def test_cfg_validator():
    from semivl_amd.monitor import PseudoLabelMeter, pl_monitor_from_cfg
    assert pl_monitor_from_cfg({}) is None and PseudoLabelMeter.from_cfg({}, 21, "cpu") is None
    assert pl_monitor_from_cfg(dict(pl_monitor={})) == dict(conf_bins=20, gt=False)
    assert pl_monitor_from_cfg(dict(pl_monitor=dict(conf_bins=20, gt=True))) == dict(conf_bins=20, gt=True)
    assert pl_monitor_from_cfg(dict(pl_monitor=dict(conf_bins=1))) == dict(conf_bins=1, gt=False)
    for bad, word in ((True, "dict"), (None, "dict"), ([("gt", True)], "dict"), (dict(bins=20), "'bins'"),
                      (dict(conf_bins=0), "conf_bins"), (dict(conf_bins=True), "conf_bins"), (dict(conf_bins=2.0), "conf_bins"),
                      (dict(conf_bins="20"), "conf_bins"), (dict(gt=1), "gt"), (dict(gt=None), "gt")):
        with pytest.raises(ValueError, match=word):
            pl_monitor_from_cfg(dict(pl_monitor=bad))
    m = PseudoLabelMeter.from_cfg(dict(pl_monitor=dict(conf_bins=5)), 3, "cpu")
    assert (m.num_classes, m.conf_bins, m.table.numel()) == (3, 5, 13 * 3 + 10 + 1)
    for bad in (0, True, 2.5):
        with pytest.raises(ValueError, match="num_classes"):
            PseudoLabelMeter(bad, 20, "cpu")
        with pytest.raises(ValueError, match="conf_bins"):
            PseudoLabelMeter(21, bad, "cpu")


def test_augmenter_reads_the_gt_switch():
    from semivl_amd.data import GpuAugmenter
    base = dict(crop_size=64)
    assert GpuAugmenter.from_cfg(base, device="cpu").unlabeled_gt is False
    assert GpuAugmenter.from_cfg(dict(base, pl_monitor=dict(conf_bins=10)), device="cpu").unlabeled_gt is False
    assert GpuAugmenter.from_cfg(dict(base, pl_monitor=dict(gt=True)), device="cpu").unlabeled_gt is True
    assert GpuAugmenter(64, device="cpu").unlabeled_gt is False
    with pytest.raises(ValueError, match="pl_monitor"):
        GpuAugmenter.from_cfg(dict(base, pl_monitor=dict(gt="yes")), device="cpu")
