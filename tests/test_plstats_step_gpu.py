"""semivl_train_step(..., monitor=PseudoLabelMeter) on the tiny VLG model of the other step tests, exact fp32 GEMMs (mode 0)
and the split emulation (mode 6): guided, with maskclip_consistency_lambda = 0, and with a label-supplying EmaTeacher.  The
meter's table equals the restatement (tests/plstats_ref.py) applied to the maps the step returns in `aux`, its loss means
equal the returned losses, and the step computes bit for bit what it computes without a meter."""
import numpy as np
import pytest
import torch

import plstats_ref as R
from test_ema_step_gpu import ADAMW, AUX_KEYS, CFG, _batch, _bits, _tiny

pytestmark = pytest.mark.gpu
BINS = 20


@pytest.fixture(params=[0, 6])
def mode(request):
    from semivl_amd import ops
    ops.set_gemm_emulation(request.param)
    yield request.param
    ops.set_gemm_emulation(0)


def _mask_u(batch, N, seed):
    """A held-back annotation for the first unlabelled view: blocks of classes, some void, the loader's 254 on the padding."""
    ign = batch["ignore_mask"]
    B, H, W = ign.shape
    g = torch.Generator().manual_seed(seed)
    small = torch.randint(0, N, (B, (H + 7) // 8, (W + 7) // 8), generator=g)
    m = small.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].clone()
    m[torch.rand(B, H, W, generator=g) < 0.05] = 255
    m = m.to(ign.device)
    m[ign == 255] = 254
    return m.contiguous()


def _setup(dev, variant):
    from semivl_amd.ema import EmaTeacher
    from semivl_amd.optim import optimizer_from_cfg
    hip, z, c = _tiny(dev)
    ocfg = dict(optimizer=ADAMW)
    if variant == "teacher":
        ocfg["ema"] = dict(decay=0.99)
    opt = optimizer_from_cfg(hip, ocfg)
    teacher = EmaTeacher.from_cfg(hip, opt, ocfg) if variant == "teacher" else None
    assert (teacher is not None and teacher.labels) == (variant == "teacher")
    cfg = dict(CFG, maskclip_consistency_lambda=0) if variant == "unguided" else CFG
    return hip, opt, teacher, cfg, z, c


def _step(dev, variant, with_meter, steps=1):
    from semivl_amd.monitor import PseudoLabelMeter
    from semivl_amd.train import semivl_train_step
    hip, opt, teacher, cfg, z, c = _setup(dev, variant)
    N = hip.num_classes
    meter = PseudoLabelMeter(N, BINS, device=dev) if with_meter else None
    out = []
    for t in range(1, steps + 1):
        batch, masks = _batch(dev, z, c)
        batch["mask_u"] = _mask_u(batch, N, 5 + t)
        losses, aux = semivl_train_step(hip, batch, t, 50, cfg, optimizer=opt, fp_masks=masks, return_aux=True,
                                        teacher=teacher, monitor=meter)
        torch.cuda.synchronize()
        out.append((losses.clone(), aux, batch))
    return out, opt.p.clone(), meter, N


def _want(aux, batch, N, thresh):
    return R.pl_stats_ref(aux["mask_w"], aux["conf_w"], batch["ignore_mask"], N, BINS, thresh, mc=aux["mclip"],
                          gt=batch["mask_u"])


@pytest.mark.parametrize("variant", ["guided", "unguided", "teacher"])
def test_meter_counts_what_the_step_trains_on(dev, mode, variant):
    from semivl_amd.train import LOSS_NAMES
    (plain,), p_plain, _, _ = _step(dev, variant, False)
    (metered,), p_metered, meter, N = _step(dev, variant, True)
    losses, aux, batch = metered
    # 1. the step itself is untouched: losses, gradients of both logit tensors, updated parameters
    assert _bits(losses, plain[0]) and _bits(aux["dl4"], plain[1]["dl4"]) and _bits(aux["dls"], plain[1]["dls"])
    assert _bits(p_metered, p_plain)
    assert set(aux) == set(plain[1]) and set(aux) - {"pred_w_teacher", "grad_stats"} == AUX_KEYS, "aux gets no new key"
    # 2. the table is the restatement on the maps the step trained on
    assert (aux["mclip"] is None) == (variant == "unguided")
    want = _want(aux, batch, N, CFG["conf_thresh"])
    assert torch.equal(meter.table, want)
    assert ("pred_w_teacher" in aux) == (variant == "teacher")      # then mask_w / conf_w / are the teacher's maps
    rep = meter.report()
    assert rep["steps"] == 1 and rep["pixels"] == batch["ignore_mask"].numel()
    assert np.array_equal(rep["table"], want.cpu().numpy())
    # 3. the loss means are the returned losses
    assert [rep["train/" + n_] for n_ in LOSS_NAMES] == losses.double().cpu().tolist()
    valid = int((batch["ignore_mask"] != 255).sum())
    assert int(rep["table"][:N].sum()) == valid and 0 < rep["mask_ratio"] <= 1
    assert "pl_miou" in rep and "guidance_miou" in rep and not np.isnan(rep["guidance_coverage"])
    if variant == "unguided":
        assert rep["guidance_coverage"] == 0.0 and np.isnan(rep["guidance_agreement"]) and np.isnan(rep["guidance_miou"])
    else:
        assert int(rep["table"][2 * N:3 * N].sum()) == int((aux["mclip"] != 255).sum())


def test_report_after_two_steps_is_the_sum(dev):
    from semivl_amd import ops
    from semivl_amd.train import LOSS_NAMES
    ops.set_gemm_emulation(0)
    out, _, meter, N = _step(dev, "guided", True, steps=2)
    want = sum(_want(aux, batch, N, CFG["conf_thresh"]) for _, aux, batch in out)
    rep = meter.report()
    assert rep["steps"] == 2 and np.array_equal(rep["table"], want.cpu().numpy())
    assert not torch.equal(out[0][1]["mask_w"], out[1][1]["mask_w"]) or not _bits(out[0][0], out[1][0])
    mean = (out[0][0].double() + out[1][0].double()).cpu().numpy() / 2.0
    assert [rep["train/" + n_] for n_ in LOSS_NAMES] == mean.tolist()
    again = meter.report()
    assert np.array_equal(again["table"], rep["table"]) and again["steps"] == 2, "report() changes nothing"


def test_monitor_none_and_missing_mask_u(dev):
    """Without `mask_u` in the batch the annotation rows stay empty; the supervised step has no `monitor` argument."""
    import inspect
    from semivl_amd.monitor import PseudoLabelMeter
    from semivl_amd.train import semivl_train_step, supervised_train_step
    from semivl_amd import ops
    ops.set_gemm_emulation(0)
    hip, opt, teacher, cfg, z, c = _setup(dev, "guided")
    N = hip.num_classes
    meter = PseudoLabelMeter(N, BINS, device=dev)
    batch, masks = _batch(dev, z, c)
    assert "mask_u" not in batch and len(batch) == 12
    losses, aux = semivl_train_step(hip, batch, 1, 50, cfg, optimizer=opt, fp_masks=masks, return_aux=True, monitor=meter)
    want = R.pl_stats_ref(aux["mask_w"], aux["conf_w"], batch["ignore_mask"], N, BINS, cfg["conf_thresh"], mc=aux["mclip"])
    assert torch.equal(meter.table, want) and not want[4 * N:13 * N].any()
    assert "pl_miou" not in meter.report()
    assert "monitor" in inspect.signature(semivl_train_step).parameters
    assert "monitor" not in inspect.signature(supervised_train_step).parameters
