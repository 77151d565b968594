"""CPU: the evaluation report's host half.  tests/evalreport_ref.py (the reference of the GPU tests) is held to the reference
project's own intersectionAndUnion through recorded triples (tests/golden/evalreport_cases.npz); EvalReport's metrics are
held to an independent second spelling, computed per class from boolean masks, within 1e-12 (the project's bound for
restatement-vs-float64 checks); `miou` / `iou_class` equal `evaluate`'s formula on the same counts bit for bit; the palette,
the normalisations, nan handling, the JSON round trip and every validator refusal."""
import json
import os

import numpy as np
import pytest
import torch

import evalreport_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FULL = dict(metrics=["mIoU", "mAcc", "mDice", "mFscore"], beta=1, nan_to_num=None)


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(HERE, "golden", "evalreport_cases.npz"))
    return z, [str(n) for n in z["names"]]


def _report(pred, target, K, spec=None):
    from semivl_amd.report import EvalReport
    return EvalReport(R.confusion_ref(pred, target, K).numpy(), K, spec)


def test_derived_rows_equal_the_recorded_reference_rows(cases):
    z, names = cases
    assert sorted(int(z[f"{n}/K"]) for n in names) == [1, 2, 21, 21]
    for n in names:
        K = int(z[f"{n}/K"])
        pred, target = torch.from_numpy(z[f"{n}/pred"]), torch.from_numpy(z[f"{n}/target"])
        assert pred.shape == (2, 24, 20)
        for v in (255, 254, -1):
            assert bool((target == v).any()), (n, v)
        table = R.confusion_ref(pred, target, K)
        inter, parea, tarea = R.derived_rows(table, K)
        ri, ru, rt = (torch.from_numpy(v) for v in z[f"{n}/iut"])
        assert torch.equal(inter, ri) and torch.equal(parea + tarea - inter, ru) and torch.equal(tarea, rt), n
        assert int(table.sum()) == int((target != 255).sum())
        rep = _report(pred, target, K)
        assert np.array_equal(rep.inter, ri.numpy()) and np.array_equal(rep.target_area, rt.numpy())
        assert np.array_equal(rep.pred_area + rep.target_area - rep.inter, ru.numpy())
        assert rep.confusion.shape == (K, K) and rep.table.shape == (K + 1, K + 1) and rep.table.dtype == np.int64
    edges = R.confusion_ref(torch.from_numpy(z["voc_edges/pred"]), torch.from_numpy(z["voc_edges/target"]), 21).view(22, 22)
    assert int(edges[21].sum()) > 0 and int(edges[:, 21].sum()) > 0          # the extra row and column are in use


def _second_spelling(pred, target, K, beta):
    """Every metric per class from boolean masks, in Python floats."""
    p, t = pred.reshape(-1).numpy(), target.reshape(-1).numpy()
    keep = t != 255
    out = {k: [] for k in ("IoU", "Acc", "Dice", "Fscore", "Precision", "Recall")}
    hit = tot = 0
    nan = float("nan")
    for k in range(K):
        I = int((keep & (p == k) & (t == k)).sum())
        P = int((keep & (p == k)).sum())
        T = int((keep & (t == k)).sum())
        hit, tot = hit + I, tot + T
        prec = I / P if P else nan
        rec = I / T if T else nan
        out["IoU"].append(100.0 * I / (P + T - I) if P + T - I else nan)
        out["Acc"].append(100.0 * rec)
        out["Recall"].append(100.0 * rec)
        out["Precision"].append(100.0 * prec)
        out["Dice"].append(100.0 * 2 * I / (P + T) if P + T else nan)
        den = beta * beta * prec + rec
        out["Fscore"].append(100.0 * (1 + beta * beta) * prec * rec / den if den == den and den != 0 else nan)
    res = {k: np.array(v) for k, v in out.items()}
    for k in list(res):
        ok = [x for x in res[k] if x == x]
        res["m" + k] = sum(ok) / len(ok) if ok else nan
    res["aAcc"] = 100.0 * hit / tot if tot else nan
    return res


@pytest.mark.parametrize("beta", [1, 0.5, 2])
def test_metrics_equal_a_second_spelling(cases, beta):
    z, names = cases
    for n in names:
        K = int(z[f"{n}/K"])
        pred, target = torch.from_numpy(z[f"{n}/pred"]), torch.from_numpy(z[f"{n}/target"])
        rep = _report(pred, target, K, dict(FULL, beta=beta))
        got, want = rep.metrics(), _second_spelling(pred, target, K, beta)
        ref = R.metrics_ref(rep.inter, rep.pred_area, rep.target_area, FULL["metrics"], beta)
        assert sorted(got) == sorted(want) == sorted(ref)
        for k in want:
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-12, equal_nan=True), (n, k, got[k], want[k])
            assert np.allclose(ref[k], want[k], rtol=0, atol=1e-12, equal_nan=True), (n, k)
        assert np.array_equal(got["Acc"], got["Recall"], equal_nan=True)
    # only the requested families appear
    rep = _report(pred, target, K, dict(metrics=("mDice",)))
    assert sorted(rep.metrics()) == ["Dice", "aAcc", "mDice"]
    assert sorted(_report(pred, target, K).metrics()) == ["IoU", "aAcc", "mIoU"]


def test_miou_is_evaluates_formula_bit_for_bit(cases):
    z, names = cases
    for n in names:
        K = int(z[f"{n}/K"])
        pred, target = torch.from_numpy(z[f"{n}/pred"]), torch.from_numpy(z[f"{n}/target"])
        rep = _report(pred, target, K)
        inter, parea, tarea = R.derived_rows(R.confusion_ref(pred, target, K), K)
        h = torch.cat([inter, parea, tarea]).numpy().astype(np.float64)          # evaluate()'s lines on its 3K histogram
        i_, u_ = h[:K], h[K:2 * K] + h[2 * K:] - h[:K]
        iou = i_ / (u_ + 1e-10) * 100.0
        assert np.array_equal(rep.iou_class, iou) and rep.miou == float(np.mean(iou))
        assert isinstance(rep.miou, float)


def test_voc_palette_against_the_fixture(cases):
    from semivl_amd.report import voc_palette
    z, _ = cases
    ref = z["pascal_palette"]
    pal = np.array(voc_palette(256)).reshape(256, 3)
    assert pal.min() >= 0 and pal.max() <= 255 and len(voc_palette()) == 768
    assert np.array_equal(pal[:21], ref[:21]) and np.array_equal(pal[255], ref[255])
    assert voc_palette(3) == [0, 0, 0, 128, 0, 0, 0, 128, 0]
    assert len({tuple(c) for c in pal.tolist()}) == 256          # a colour per index, not white from 21 on


def test_normalized_nan_and_nan_to_num():
    # class 2 never annotated and never predicted, class 3 predicted but never annotated
    target = torch.tensor([0, 0, 0, 1, 1, 255, 254, 0])
    pred = torch.tensor([0, 0, 1, 1, 3, 0, 1, 9])
    rep = _report(pred, target, 4, FULL)
    assert rep.table[4].tolist() == [0, 1, 0, 0, 0] and rep.table[:, 4].tolist() == [1, 0, 0, 0, 0]
    c = rep.confusion.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        want_t, want_p = c / c.sum(1, keepdims=True), c / c.sum(0, keepdims=True)
    assert np.array_equal(rep.normalized("target"), want_t, equal_nan=True) and np.isnan(rep.normalized("target")[2]).all()
    assert np.array_equal(rep.normalized("pred"), want_p, equal_nan=True) and np.isnan(rep.normalized("pred")[:, 2]).all()
    assert np.array_equal(rep.normalized("all"), c / c.sum()) and rep.normalized() is not None
    with pytest.raises(ValueError, match="over"):
        rep.normalized("rows")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = rep.metrics()
    assert np.isnan(m["IoU"][2]) and np.isnan(m["Acc"][2]) and np.isnan(m["Acc"][3]) and m["IoU"][3] == 0.0
    assert np.isnan(m["Precision"][2]) and m["Precision"][3] == 0.0 and np.isnan(m["Fscore"][3]) and np.isnan(m["Dice"][2])
    assert m["mAcc"] == pytest.approx((200.0 / 4 + 100.0 / 2) / 2, abs=1e-12)          # nanmean over the two annotated classes
    assert m["aAcc"] == pytest.approx(100.0 * 3 / 6, abs=1e-12)
    z = _report(pred, target, 4, dict(FULL, nan_to_num=-1)).metrics()
    assert z["IoU"][2] == -1 and z["Acc"][3] == -1 and not any(np.isnan(v).any() for v in z.values())
    assert np.array_equal(np.nan_to_num(m["IoU"], nan=-1.0), z["IoU"]) and z["mIoU"] == m["mIoU"]
    empty = _report(torch.tensor([0, 1]), torch.tensor([255, 255]), 2, dict(FULL, nan_to_num=0))
    assert empty.metrics()["aAcc"] == 0 and empty.metrics()["mIoU"] == 0 and empty.miou == 0.0
    assert np.isnan(_report(torch.tensor([0, 1]), torch.tensor([255, 255]), 2).metrics()["aAcc"])


def test_to_dict_round_trips_and_table_prints(cases):
    z, _ = cases
    pred, target = torch.from_numpy(z["voc/pred"]), torch.from_numpy(z["voc/target"])
    rep = _report(pred, target, 21, FULL)
    d = rep.to_dict()
    assert json.loads(json.dumps(d, allow_nan=False)) == d
    assert d["nclass"] == 21 and d["miou"] == rep.miou and d["table"] == rep.table.tolist()
    assert d["metrics"]["mDice"] == rep.metrics()["mDice"] and d["spec"]["metrics"] == FULL["metrics"]
    assert _report(torch.tensor([0]), torch.tensor([1]), 3, FULL).to_dict()["metrics"]["IoU"][2] is None
    txt = rep.format_table()
    lines = txt.splitlines()
    assert len(lines) == 21 + 3 and lines[0].split() == ["Class", "IoU", "Acc", "Dice", "Fscore", "Precision", "Recall"]
    assert lines[1].split()[1] == f"{rep.metrics()['IoU'][0]:.2f}"
    assert lines[-1].split() == [f"{rep.metrics()[k]:.2f}" for k in ("aAcc", "mIoU", "mAcc", "mDice", "mFscore", "mPrecision",
                                                                    "mRecall")]
    names = [f"c{i}" for i in range(21)]
    assert rep.format_table(names).splitlines()[21].split()[0] == "c20"
    with pytest.raises(ValueError, match="class names"):
        rep.format_table(names[:-1])


def test_validator_refusals_name_the_offender():
    from semivl_amd.report import EvalReport, _check_palette, eval_report_from_cfg
    assert eval_report_from_cfg({}) is None
    assert eval_report_from_cfg(dict(eval_report={})) == dict(metrics=("mIoU",), beta=1.0, nan_to_num=None)
    assert eval_report_from_cfg(dict(eval_report=FULL)) == dict(metrics=tuple(FULL["metrics"]), beta=1.0, nan_to_num=None)
    assert eval_report_from_cfg(dict(eval_report=dict(beta=0.5, nan_to_num=0)))["nan_to_num"] == 0.0
    bad = [(None, "dict"), ([("metrics", [])], "dict"), ("mIoU", "dict"), (dict(metric=["mIoU"]), "'metric'"),
           (dict(metrics="mIoU"), "metrics"), (dict(metrics=["mIoU", "mBoundary"]), "'mBoundary'"), (dict(metrics=[3]), "3"),
           (dict(beta=0), "beta 0"), (dict(beta=-1.0), "beta -1.0"), (dict(beta=True), "beta True"),
           (dict(beta="1"), "beta '1'"), (dict(beta=float("nan")), "beta nan"), (dict(nan_to_num=False), "nan_to_num False"),
           (dict(nan_to_num="0"), "nan_to_num '0'")]
    for spec, word in bad:
        with pytest.raises(ValueError, match="eval_report.*" + word):
            eval_report_from_cfg(dict(eval_report=spec))
    assert _check_palette(None) == _check_palette(tuple(_check_palette(None))) and _check_palette([]) == []
    assert _check_palette(np.arange(6, dtype=np.uint8)) == [0, 1, 2, 3, 4, 5]
    for pal, word in ((list(range(4)), "length 4"), ([0] * 771, "length 771"), ([0, 0, 256], "256"), ([0, 0, -1], "-1"),
                      ([0, 0, 1.5], "1.5"), ([0, 0, True], "True"), ("abc", "str"), (7, "int")):
        with pytest.raises(ValueError, match="palette.*" + word):
            _check_palette(pal)
    with pytest.raises(ValueError, match="table"):
        EvalReport(np.zeros(9, np.int64), 3)
    with pytest.raises(ValueError, match="table"):
        EvalReport(np.zeros(16, np.float64), 3)
