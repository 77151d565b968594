"""The OHEM supervised criterion (cfg['criterion'] = 'OHEM', third_party/unimatch/util/ohem.py) without a GPU: how the
step reads the configuration, the constructor of the reference-named module, and ohem_cases.npz (recorded from the
reference's own ProbOhemCrossEntropy2d) against a float64 restatement of what the criterion computes."""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from semivl_amd.train import ProbOhemCrossEntropy2d, supervised_criterion

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ohem_cases.npz")


def test_criterion_parsing_defaults():
    assert supervised_criterion({}) is None
    assert supervised_criterion(dict(criterion=dict(name="CELoss", kwargs=dict(ignore_index=255)))) is None
    assert supervised_criterion(dict(criterion=dict(name="mmseg", kwargs={}))) is None      # (unchanged: plain CE)
    c = supervised_criterion(dict(criterion=dict(name="OHEM", kwargs=dict(ignore_index=255))))
    assert isinstance(c, ProbOhemCrossEntropy2d)
    assert (c.thresh, c.min_kept) == (0.7, 256)          # ohem.py's defaults: experiments.py:231's kwargs never arrive
    c = supervised_criterion(dict(criterion=dict(name="OHEM", kwargs=dict(ignore_index=255, thresh="0.5", min_kept=2e5,
                                                                        down_ratio=8))))
    assert (c.thresh, c.min_kept, c.down_ratio) == (0.5, 200000, 8)


def test_criterion_parsing_refusals():
    def mk(**kw):
        return supervised_criterion(dict(criterion=dict(name="OHEM", kwargs=dict(dict(ignore_index=255), **kw))))
    with pytest.raises(NotImplementedError, match="use_weight"):
        mk(use_weight=True)
    with pytest.raises(NotImplementedError, match="reduction"):
        mk(reduction="none")
    with pytest.raises(ValueError, match="ignore_index"):
        mk(ignore_index=-100)
    with pytest.raises(TypeError):
        supervised_criterion(dict(criterion=dict(name="OHEM", kwargs={})))   # ignore_index has no default in ohem.py


def test_constructor_signature():
    sig = inspect.signature(ProbOhemCrossEntropy2d.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("ignore_index", inspect.Parameter.empty), ("reduction", "mean"), ("thresh", 0.7), ("min_kept", 256),
        ("down_ratio", 1), ("use_weight", False)]
    assert issubclass(ProbOhemCrossEntropy2d, torch.nn.Module)


def restate(logits, target, H, W, align, thresh, min_kept):
    """ohem.py in float64: (relabelled target, mean CE over the kept pixels, d(loss)/d(low-resolution logits))."""
    x = logits.double().requires_grad_(True)
    full = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=align)
    valid = target != 255
    nv = int(valid.sum())
    p = F.softmax(full, dim=1).gather(1, (target * valid).unsqueeze(1)).squeeze(1)
    p = torch.where(valid, p, torch.ones_like(p)).detach()
    keep = valid.clone()
    if not min_kept > nv and nv > 0 and min_kept > 0:     # (min_kept == 0: ohem.py keeps every valid pixel)
        v = p.flatten().kthvalue(min(p.numel(), min_kept)).values
        t = v if v > thresh else torch.tensor(thresh, dtype=torch.float64)
        keep &= p <= t
    relabel = torch.where(keep, target, torch.full_like(target, 255))
    loss = F.cross_entropy(full, relabel, ignore_index=255)
    loss.backward()
    return relabel, loss.item(), x.grad


def test_cases_match_float64_restatement():
    z = np.load(GOLDEN)
    names = []
    for i in range(int(z["num_cases"])):
        pre = f"c{i}/"
        H, W, align = (int(v) for v in z[pre + "geom"])
        target = torch.from_numpy(z[pre + "target"].astype(np.int64))
        relabel, loss, grad = restate(torch.from_numpy(z[pre + "logits"]), target, H, W, bool(align),
                                      float(z[pre + "thresh"]), int(z[pre + "min_kept"]))
        name = str(z[pre + "name"])
        names.append(name)
        assert np.array_equal(relabel.numpy().astype(np.uint8), z[pre + "relabel"]), name
        assert abs(loss - float(z[pre + "loss"])) < 1e-5 * abs(float(z[pre + "loss"])), name
        g = z[pre + "grad"]
        assert np.abs(grad.numpy() - g).max() < 1e-5 * np.abs(g).max(), name
        kept, nv = int((relabel != 255).sum()), int((target != 255).sum())
        mk = int(z[pre + "min_kept"])
        if name in ("kth_binds", "heavy_ignore"):
            assert kept == mk                   # the k-th value binds: exactly min_kept pixels (no ties there)
        if name == "thresh_binds" or name == "ties":
            assert mk < kept < nv
        if name in ("min_kept_gt_valid", "min_kept_zero", "min_kept_gt_numel"):
            assert kept == nv
    assert len(names) == 7
