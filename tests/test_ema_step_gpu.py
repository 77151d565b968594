"""The mean teacher (semivl_amd/ema.py) through the optimizers, the two training steps, the evaluator and the checkpoint on
the tiny VLG model (the fixture of tests/test_gradclip_step_gpu.py) and the tiny DeepLabV3+ `ftap` model with train-mode
BatchNorm (tests/test_dlv3p_gpu.py), exact fp32 GEMMs (mode 0) and the split emulation (mode 6), at most 3 steps each.
Averages and BatchNorm statistics are held to the float64 restatement (tests/ema_ref.py) under the kernel tests' bound:
gamma(n) (|d32 a| + |omd32 b|) per step -- n = 3 for the step kernels' expression, 2 for svl_ema_segments_f32 --
R.compounded_bound over several."""
import numpy as np
import pytest
import torch

import ema_ref as R
from golden_util import build_hip, fixture_batch, fixture_fp_masks, fixture_state, load_fixture
from test_dlv3p_gpu import C1, C4, STEP_CFG, _tiny_model

pytestmark = pytest.mark.gpu

CFG = dict(conf_thresh=0.05, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
           maskclip_consistency_lambda=[0.1, 0], fuse_upsample_loss=True)
ADAMW = dict(type="AdamW", lr=1e-3, weight_decay=0.01)
AUX_KEYS = {"mask_w", "mask_w_other", "mclip", "mclip_other", "conf_w", "pred_x", "pred_s1", "pred_w", "pred_w_other", "dl4",
            "dls", "upsample_in_loss", "mask_x_ohem"}                 # what the step returned before it knew a teacher
LOGIT_TOL = 1e-3                                                       # the model tests' logit limit


@pytest.fixture(params=[0, 6])
def mode(request):
    from semivl_amd import ops
    ops.set_gemm_emulation(request.param)
    yield request.param
    ops.set_gemm_emulation(0)


def _tiny(dev):
    z, c = load_fixture("tiny")
    hip = build_hip(c)
    hip.load_state_dict(fixture_state(z, c, hip), strict=True)
    return hip.to(dev), z, c


def _batch(dev, z, c):
    """A fresh copy: the step cuts img_s1 / img_s2 in place."""
    return {k: v.clone().to(dev) for k, v in fixture_batch(z, c).items()}, [m.to(dev) for m in fixture_fp_masks(z, c)]


def _vlg(dev, ema, optimizer=ADAMW, **teacher_kw):
    """(model, optimizer, teacher, z, c) of a fresh tiny VLG model; `ema`: cfg['ema']."""
    from semivl_amd.ema import EmaTeacher
    from semivl_amd.optim import optimizer_from_cfg
    hip, z, c = _tiny(dev)
    cfg = dict(optimizer=optimizer, ema=ema) if optimizer is not None else dict(lr=2.0 ** -10, lr_multi=10.0, ema=ema)
    opt = optimizer_from_cfg(hip, cfg)
    return hip, opt, EmaTeacher.from_cfg(hip, opt, dict(cfg, **teacher_kw)), z, c


def _bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _within(got, ref, bound):
    """Worst |got - ref| / bound; where the bound is 0 (the arena's padding: 0 = d 0 + (1 - d) 0) the result is exact."""
    err = np.abs(got.double().cpu().numpy().reshape(-1) - ref.reshape(-1))
    bound = bound.reshape(-1)
    live = bound > 0
    assert not err[~live].any()
    return float((err[live] / bound[live]).max())


# ------------------------------------------------------------------------------------------------ 1. structure
def _check_structure(student, opt, teacher, before, n_tables):
    t = teacher.model
    assert type(t) is type(student) and not any(m.training for m in t.modules())
    assert t.train() is t and not t.training and not any(p.requires_grad for p in t.parameters())
    assert list(t.state_dict()) == list(student.state_dict())
    slot = {id(g_["param"]): i for i, g_ in enumerate(opt.groups)}
    sp, tp = dict(student.named_parameters()), dict(t.named_parameters())
    assert list(sp) == list(tp)
    n_arena = 0
    for name, p in sp.items():
        if id(p) in slot:
            off = opt._offs[slot[id(p)]]
            assert tp[name].data_ptr() == opt.ema.data_ptr() + 4 * off and tp[name].shape == p.shape, name
            assert tp[name].data_ptr() != p.data_ptr()
            n_arena += 1
        else:       # shared: the student's object, or (clip_encoder.*, registered as trainable but never trained) its storage
            assert tp[name].data_ptr() == p.data_ptr() and (tp[name] is p or p.requires_grad), name
    assert n_arena == len(opt.groups) == len(teacher.arena_params()) > 0
    assert all(tp[n_].data_ptr() == p.data_ptr() for n_, p in sp.items() if n_.startswith("clip_encoder."))
    sb, tb = dict(student.named_buffers()), dict(t.named_buffers())
    assert list(sb) == list(tb)
    own = 0
    for name, b in sb.items():
        if name.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked"):
            assert tb[name].data_ptr() != b.data_ptr() and _bits(tb[name], b), name
            own += tb[name].numel() * tb[name].element_size()
        else:
            assert tb[name] is b, name
    assert t.loaded_mcc_text_feat is student.loaded_mcc_text_feat
    # memory: the BatchNorm buffers' bytes, the pointer tables and one allocator block.  Granularity: torch's caching
    # allocator hands out multiples of 512 B, so `one block` is 512 B.  (The teacher's statistics are ONE flat tensor and the
    # student's per-module counters, a 512 B block each, move into one flat tensor as well: measured 5632 B for 7624 B of
    # own buffers on the DLV3P model, 0 B on the VLG model.)
    n_bn = sum(1 for n_ in sb if n_.endswith("running_mean"))
    allowed = own + n_tables * 8 * (2 * n_bn + 1) + 512
    grown = torch.cuda.memory_allocated() - before
    print(f"EmaTeacher: memory_allocated grew by {grown} B (allowed {allowed} B; own BatchNorm buffers {own} B)")
    assert grown <= allowed
    return own


def test_structure_vlg(dev):
    from semivl_amd.ema import EmaTeacher
    from semivl_amd.train import FusedAdamW
    hip, _, _ = _tiny(dev)
    opt = FusedAdamW(hip, ADAMW, ema_decay=0.99)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    teacher = EmaTeacher(hip, opt)
    assert _check_structure(hip, opt, teacher, before, 0) == 0 and teacher.labels and teacher.buffers == "ema"
    assert opt.ema_warmup is False and opt.ema_decay_at(1) == 0.99          # ema_decay= alone: constant, as before
    with pytest.raises(ValueError, match="EMA arena"):
        EmaTeacher(hip, FusedAdamW(_tiny(dev)[0], ADAMW))
    with pytest.raises(ValueError, match="buffers"):
        EmaTeacher(hip, opt, buffers="mean")


def test_structure_dlv3p(dev, tmp_path, monkeypatch):
    from semivl_amd.ema import EmaTeacher
    from semivl_amd.optim import optimizer_from_cfg
    model, cfg = _tiny_model(tmp_path, monkeypatch, dev)
    opt = optimizer_from_cfg(model, dict(cfg, ema=dict(decay=0.996)))
    assert opt.ema is not None and opt.ema_warmup and opt.ema_decay == 0.996 and opt.ema_decay_at(2) == 0.5
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    teacher = EmaTeacher.from_cfg(model, opt, dict(cfg, ema=dict(decay=0.996)))
    assert _check_structure(model, opt, teacher, before, 3) > 0
    assert EmaTeacher.from_cfg(model, opt, cfg) is None


# ------------------------------------------------------------------------------------------------ 2. the average
@pytest.mark.parametrize("kind", ["adamw-warmup", "sgd-constant"])
def test_average_follows_the_restated_recursion(dev, mode, kind):
    from semivl_amd.train import semivl_train_step
    warm = kind == "adamw-warmup"
    hip, opt, teacher, z, c = _vlg(dev, dict(decay=0.996, warmup=warm), ADAMW if warm else None)
    start = opt.ema.double().cpu().numpy()
    assert np.array_equal(start, opt.p.double().cpu().numpy())
    ps, prev, worst = [], start, 0.0
    for t in (1, 2, 3):
        batch, masks = _batch(dev, z, c)
        semivl_train_step(hip, batch, t, 50, CFG, optimizer=opt, fp_masks=masks, teacher=teacher)
        torch.cuda.synchronize()
        d = R.schedule(0.996, warm, t)
        assert opt.step_count == t and opt.ema_decay_at(t) == d
        ps.append(opt.p.double().cpu().numpy())
        ref, bound = R.step_ref(prev, ps[-1], d)
        worst = max(worst, _within(opt.ema, ref, bound))
        prev = opt.ema.double().cpu().numpy()
        if warm and t == 1:
            assert np.array_equal(prev, ps[0]), "d_1 = 0: the average starts as the first updated weights"
    print(f"{kind} mode {mode}: one-step relation, worst error / bound = {worst:.3f}")
    assert worst <= 1.0 and not np.array_equal(ps[0], ps[2])
    if warm:
        mean = (ps[0] + ps[1] + ps[2]) / 3.0
        r3 = _within(opt.ema, mean, R.compounded_bound(ps, 0.996, True, start))
        print(f"{kind} mode {mode}: mean of three steps, error / compounded bound = {r3:.3f}")
        assert r3 <= 1.0
    # the teacher's tensors ARE the arena: no copy was needed
    for ai, tp in teacher.arena_params():
        assert _bits(tp.detach(), opt._seg(opt.ema, ai))


# ------------------------------------------------------------------------------------------------ 3. BatchNorm buffers
def _bn_buffers(model):
    return {n_: b.detach().clone() for n_, b in model.named_buffers() if n_.rsplit(".", 1)[-1] in
            ("running_mean", "running_var", "num_batches_tracked")}


@pytest.mark.parametrize("buffers,labels", [("ema", True), ("copy", False)])
def test_batchnorm_buffers_follow_the_student(dev, mode, tmp_path, monkeypatch, buffers, labels):
    """buffers='ema': the float64 recursion over the student's recorded statistics.  buffers='copy' with teacher=False in the
    configuration: the student's bits, and the labels are the student's -- the teacher is only maintained."""
    from semivl_amd.ema import EmaTeacher
    from semivl_amd.optim import optimizer_from_cfg
    from semivl_amd.synthetic import synthetic_batch
    from semivl_amd.train import semivl_train_step
    B, S_, N = 2, 64, 5
    model, cfg = _tiny_model(tmp_path, monkeypatch, dev, S_, N)
    cfg = dict(cfg, ema=dict(decay=0.996, buffers=buffers, teacher=labels))
    opt = optimizer_from_cfg(model, cfg)
    teacher = EmaTeacher.from_cfg(model, opt, cfg)
    assert teacher.labels is labels and teacher.buffers == buffers
    prev, worst = _bn_buffers(teacher.model), 0.0
    ema0 = opt.ema.clone()
    for t in (1, 2):
        batch = synthetic_batch(B, S_, N, seed=98 + t, device=dev)
        fp_masks = [(torch.rand(2 * B, ch, generator=torch.Generator().manual_seed(7 + ch + t)) < 0.5).float().to(dev)
                    for ch in (C1, C4)]
        _, aux = semivl_train_step(model, batch, t, 10, STEP_CFG, optimizer=opt, fp_masks=fp_masks, teacher=teacher,
                                   return_aux=True)
        torch.cuda.synchronize()
        assert ("pred_w_teacher" in aux) is labels
        stu, tea = _bn_buffers(model), _bn_buffers(teacher.model)
        d = R.schedule(0.996, True, t)
        for name, s in stu.items():
            if name.endswith("num_batches_tracked"):
                assert int(tea[name]) == int(s) == 2 * t, name
            elif buffers == "copy":
                assert _bits(tea[name], s), name
            else:
                ref, bound = R.step_ref(prev[name].double().cpu().numpy(), s.double().cpu().numpy(), d,
                                        n=R.N_ROUNDINGS_SEGMENTS)
                worst = max(worst, _within(tea[name], ref, bound))
                if t == 2:
                    assert not _bits(tea[name], s), name
        prev = tea
    print(f"DLV3P buffers={buffers} mode {mode}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0 and not torch.equal(opt.ema, ema0), "the average is maintained either way"


# ------------------------------------------------------------------------------------------------ 4. labels
def _teacher_labels(teacher, student, batch, cfg):
    """What the step must compute: teacher.model(cat(img_w, img_w_other)) with the step's own resize choice, then its
    softmax-max."""
    from semivl_amd import ops
    from semivl_amd.train import _head_res
    up = _head_res(student, batch["img_x"], cfg)
    with torch.no_grad():
        pred = teacher.model(torch.cat((batch["img_w"], batch["img_w_other"])), **(dict(head_res=True) if up else {}))
        conf, mask = ops.softmax_max_up(pred, *up) if up is not None else ops.softmax_max(pred)
        if up is not None:
            pred = ops.bilinear_planes_fwd(pred.contiguous(), pred.shape[2], pred.shape[3], up[2], up[0], up[1])
    return up, pred, conf, mask


@pytest.mark.parametrize("fuse", [True, False])
def test_labels_come_from_the_teacher(dev, mode, fuse):
    from semivl_amd import ops
    from semivl_amd.train import semivl_train_step
    cfg = dict(CFG, fuse_upsample_loss=fuse)
    hip, opt, teacher, z, c = _vlg(dev, dict(decay=0.5, warmup=False))
    twin, topt, _, _, _ = _vlg(dev, dict(decay=0.5, warmup=False))
    # a teacher that is not the student: every averaged tensor a quarter smaller
    opt.ema.mul_(0.75)
    ops.weights_changed()
    batch, masks = _batch(dev, z, c)
    B = batch["img_x"].shape[0]
    up, pred, conf, mask = _teacher_labels(teacher, hip, batch, cfg)
    assert (up is not None) is fuse
    losses, aux = semivl_train_step(hip, batch, 1, 50, cfg, optimizer=opt, fp_masks=masks, teacher=teacher, return_aux=True)
    tb, tm = _batch(dev, z, c)
    tlosses, taux = semivl_train_step(twin, tb, 1, 50, cfg, optimizer=topt, fp_masks=tm, return_aux=True)
    torch.cuda.synchronize()
    assert aux["upsample_in_loss"] is fuse and set(aux) == AUX_KEYS | {"pred_w_teacher"} and set(taux) == AUX_KEYS
    assert _bits(aux["mask_w"], mask[:B]) and _bits(aux["mask_w_other"], mask[B:]) and _bits(aux["conf_w"], conf[:B])
    assert _bits(aux["pred_w_teacher"], pred[:B]) and _bits(aux["pred_w_other"], pred[B:])
    differ = int((aux["mask_w"] != taux["mask_w"]).sum())
    print(f"mode {mode} fuse {fuse}: {differ} of {aux['mask_w'].numel()} pseudo-labels differ from the student's")
    assert differ > 0, "the teacher's labels equal the student's: the comparison above proves nothing"
    assert _bits(aux["pred_w"], taux["pred_w"]), "pred_w stays the student's"
    assert _bits(losses[1:2], tlosses[1:2]) and not _bits(losses[2:5], tlosses[2:5])


# ------------------------------------------------------------------------------------------------ 5. no stale planes
def test_teacher_planes_are_rebuilt_after_the_step(dev, mode):
    """decay = 0: after the step the teacher IS the updated student.  Its forward must equal that of a freshly built model
    loaded from teacher.model.state_dict() -- with weight planes / packs cached across the step it would still be the forward
    of the OLD weights, LOGIT_TOL x 100 away (asserted).  Held to the model tests' logit limit and not bit for bit: the fresh
    model's tensors are separate 256-byte aligned allocations, the teacher's are 16-byte aligned slices of the arena, and not
    every kernel's path choice is independent of the operand's address."""
    from semivl_amd.train import semivl_train_step
    hip, opt, teacher, z, c = _vlg(dev, dict(decay=0.0, warmup=False), dict(type="AdamW", lr=0.05, weight_decay=0.0))
    batch, masks = _batch(dev, z, c)
    img = batch["img_w"].clone()
    with torch.no_grad():
        y0 = teacher.model(img).clone()                      # fills the caches with the planes of the OLD weights
    semivl_train_step(hip, batch, 1, 50, CFG, optimizer=opt, fp_masks=masks, teacher=teacher)
    with torch.no_grad():
        y1 = teacher.model(img).clone()
    fresh = build_hip(c).to(dev)
    fresh.load_state_dict(teacher.model.state_dict(), strict=True)
    fresh.eval()
    with torch.no_grad():
        ref = fresh(img)
    torch.cuda.synchronize()
    moved, err = float((y1 - y0).abs().max()), float((y1 - ref).abs().max())
    print(f"mode {mode}: one step moved the teacher's logits by {moved:.3g}; teacher vs fresh model {err:.3g} "
          f"(bit-equal: {_bits(y1, ref)})")
    assert bool(torch.isfinite(y1).all()) and moved >= 100 * LOGIT_TOL
    assert err <= LOGIT_TOL


# ------------------------------------------------------------------------------------------------ 6. streams
def test_side_stream_pass_is_reproducible(dev, mode, tmp_path, monkeypatch):
    """The DLV3P step with a teacher (its pseudo-label pass on the second stream although the head has BatchNorm), twice from
    the same state, two steps each: losses, the average and the teacher's statistics bit for bit."""
    from semivl_amd.ema import EmaTeacher
    from semivl_amd.optim import optimizer_from_cfg
    from semivl_amd.synthetic import synthetic_batch
    from semivl_amd.train import semivl_train_step
    B, S_, N = 2, 64, 5
    runs = []
    for tag in ("a", "b"):
        (tmp_path / tag).mkdir()
        model, cfg = _tiny_model(tmp_path / tag, monkeypatch, dev, S_, N)
        cfg = dict(cfg, ema=dict(decay=0.5, warmup=False))
        opt = optimizer_from_cfg(model, cfg)
        teacher = EmaTeacher.from_cfg(model, opt, cfg)
        out = []
        for t in (1, 2):
            fp_masks = [(torch.rand(2 * B, ch, generator=torch.Generator().manual_seed(7 + ch)) < 0.5).float().to(dev)
                        for ch in (C1, C4)]
            out.append(semivl_train_step(model, synthetic_batch(B, S_, N, seed=99, device=dev), t, 10,
                                         dict(STEP_CFG, overlap_streams=True), optimizer=opt, fp_masks=fp_masks,
                                         teacher=teacher).clone())
        torch.cuda.synchronize()
        runs.append((out, opt.ema.clone(), _bn_buffers(teacher.model)))
    (la, ea, ba), (lb, eb, bb) = runs
    assert all(_bits(x, y) for x, y in zip(la, lb)) and bool(torch.isfinite(la[1]).all())
    assert _bits(ea, eb) and all(_bits(ba[k], bb[k]) for k in ba) and len(ba) > 0


# ------------------------------------------------------------------------------------------------ 7. checkpoint
def test_checkpoint_and_evaluate(dev, tmp_path):
    from semivl_amd.checkpoint import load_checkpoint, save_checkpoint
    from semivl_amd.evaluate import evaluate
    from semivl_amd.train import semivl_train_step
    hip, opt, teacher, z, c = _vlg(dev, dict(decay=0.5, warmup=False))
    batch, masks = _batch(dev, z, c)
    semivl_train_step(hip, batch, 1, 50, CFG, optimizer=opt, fp_masks=masks, teacher=teacher)
    path = str(tmp_path / "best.pth")
    ck = save_checkpoint(path, hip, opt, 3, ema_model=teacher.model)
    assert set(ck) == {"model", "optimizer", "epoch", "ema_model"} and all(k.startswith("module.") for k in ck["ema_model"])
    assert set(ck["ema_model"]) == set(ck["model"]) and set(ck["optimizer"]) == {"state", "param_groups", "names"}
    fresh = build_hip(c).to(dev)
    assert load_checkpoint(path, fresh, ema=True) == 3
    want, got = teacher.model.state_dict(), fresh.state_dict()
    keys = [k for k in want if "clip_encoder" not in k]
    assert len(keys) > 10 and all(_bits(want[k], got[k]) for k in keys)
    assert not all(_bits(want[k], hip.state_dict()[k]) for k in keys), "the average must differ from the student here"
    # a resumed run: the file's average lands in a new optimizer's arena through the teacher's views
    hip2, opt2, teacher2, _, _ = _vlg(dev, dict(decay=0.5, warmup=False))
    assert not _bits(opt2.ema, opt.ema)
    load_checkpoint(path, teacher2.model, ema=True)
    for ai in range(len(opt.groups)):
        assert _bits(opt2._seg(opt2.ema, ai), opt._seg(opt.ema, ai)), opt.groups[ai]["name"]
    # evaluate takes the teacher as any model
    g = torch.Generator().manual_seed(4)
    S_ = c["S"]
    loader = [(torch.randn(1, 3, S_, S_, generator=g), torch.randint(0, 21, (1, S_, S_), generator=g), None) for _ in range(2)]
    ecfg = dict(nclass=21, crop_size=S_)
    m_t, iou_t = evaluate(teacher.model, loader, "original", ecfg)
    m_f, iou_f = evaluate(fresh, loader, "original", ecfg)
    m_s, _ = evaluate(hip, loader, "original", ecfg)
    assert m_t == m_f and np.array_equal(iou_t, iou_f) and not teacher.model.training
    print(f"mIoU teacher {m_t:.4f}, fresh model loaded from ema_model {m_f:.4f}, student {m_s:.4f}")


# ------------------------------------------------------------------------------------------------ 8. off is off
def test_off_is_off(dev, mode):
    from semivl_amd.train import FusedAdamW, semivl_train_step, supervised_train_step
    out = []
    for kw in ({}, dict(teacher=None)):
        hip, z, c = _tiny(dev)
        opt = FusedAdamW(hip, ADAMW, ema_decay=0.99)
        batch, masks = _batch(dev, z, c)
        losses, aux = semivl_train_step(hip, batch, 1, 50, CFG, optimizer=opt, fp_masks=masks, return_aux=True, **kw)
        torch.cuda.synchronize()
        out.append((losses.clone(), aux, opt.p.clone(), opt.ema.clone()))
    (l0, a0, p0, e0), (l1, a1, p1, e1) = out
    assert _bits(l0, l1) and set(a0) == set(a1) == AUX_KEYS and _bits(p0, p1) and _bits(e0, e1)
    assert _bits(a0["mask_w"], a1["mask_w"])
    # teacher=False in the configuration: the labels are the student's, the average is still maintained
    hip, opt, teacher, z, c = _vlg(dev, dict(decay=0.99, warmup=False, teacher=False))
    assert teacher.labels is False
    batch, masks = _batch(dev, z, c)
    l2, a2 = semivl_train_step(hip, batch, 1, 50, CFG, optimizer=opt, fp_masks=masks, return_aux=True, teacher=teacher)
    torch.cuda.synchronize()
    assert _bits(l2, l0) and set(a2) == AUX_KEYS and _bits(a2["mask_w"], a0["mask_w"]) and _bits(opt.ema, e0)
    assert not _bits(opt.ema, opt.p)
    # the supervised step only maintains the teacher
    hip, opt, teacher, z, c = _vlg(dev, dict(decay=0.99, warmup=False))
    batch, _ = _batch(dev, z, c)
    before = opt.ema.clone()
    _, a3 = supervised_train_step(hip, dict(img_x=batch["img_x"], mask_x=batch["mask_x"]), 1, 50, CFG, optimizer=opt,
                                  return_aux=True, teacher=teacher)
    torch.cuda.synchronize()
    assert set(a3) == {"pred_x", "dlogits", "mask_x_ohem", "upsample_in_loss"} and not _bits(opt.ema, before)
    ref, bound = R.step_ref(before.double().cpu().numpy(), opt.p.double().cpu().numpy(), 0.99)
    assert _within(opt.ema, ref, bound) <= 1.0


# ------------------------------------------------------------------------------------------------ 9. two ranks
def _rank_worker(rank, world, port, q):
    import os
    import sys
    import torch.distributed as dist
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from semivl_amd.synthetic import synthetic_batch
    from semivl_amd.train import GradAllReducer, semivl_train_step
    hip, opt, teacher, z, c = _vlg(dev, dict(decay=0.5, warmup=False))
    red = GradAllReducer(opt, bucket_mb=0.05, overlap=True)
    red.broadcast_params()
    teacher.reset()
    masks = [m.to(dev) for m in fixture_fp_masks(z, c)]
    for t in (1, 2):        # DIFFERENT data on every rank and step
        batch = {k: v.to(dev) for k, v in synthetic_batch(c["B"], c["S"], 21, seed=500 + 10 * t + rank).items()}
        semivl_train_step(hip, batch, t, 50, CFG, optimizer=opt, reducer=red, fp_masks=masks, teacher=teacher)
    torch.cuda.synchronize()
    q.put((rank, opt.ema.cpu().numpy(), opt.p.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_average(dev):
    """Two gloo processes on the one GPU, two steps on different shards (the pattern of tests/test_multiproc_gpu.py): every
    rank holds the same weights after the all-reduce, hence the same average -- bit for bit, nothing communicated for it."""
    import os
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29300 + os.getpid() % 200
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t_: t_[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    (_, e0, p0), (_, e1, p1) = res
    assert np.array_equal(p0.view(np.int32), p1.view(np.int32)), "the ranks' weights differ: nothing to conclude"
    assert np.array_equal(e0.view(np.int32), e1.view(np.int32))
    assert not np.array_equal(e0, p0)
