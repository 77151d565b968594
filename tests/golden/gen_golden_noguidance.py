"""Golden-vector generator for training WITHOUT MaskCLIP guidance (experiment 41's rows: `clip_encoder=None`,
`maskclip_consistency_lambda=0`, `mcc_loss_reduce='mean'`) and for the labelled-only baseline (method 'supervised').
Runs ONLY where the reference tree exists, like gen_golden.py: it builds the reference's own VLM from the VLG config with
`clip_encoder=None` at the 'tiny' fixture dimensions and drives it, in FLOAT64 (parameters, inputs and the default dtype
are float64, and the `.float()` casts inside the reference keep float64 for the duration of the run), with the restated
loop bodies of tests/noguidance_ref.py -- semivl.py:223-328 along its `lambda == 0` branches with the reference's own
cutmix_* / confidence_weighted_loss helpers, and supervised.py:277-289 -- and writes tests/golden/semivl_noguidance.npz.

    python tests/golden/gen_golden_noguidance.py

Case A: one semi-supervised step, conf_mode 'pixelwise'.  As in gen_golden.py's 'vlgdim' / 'conf' fixtures the predictions
        are peaked (decoder's last conv x 150, low-passed inputs) and conf_thresh sits in the middle of the widest gap
        between any two pixel confidences inside their 25 % ... 75 % quantile range, which must be >= 2e-4: the three
        unlabelled branches are live and no legitimate change of the forward rounding moves a pixel across the gate.
Case C: one supervised step of the same model with nn.CrossEntropyLoss(ignore_index=255).
Case B: the DeepLabV3+ `ftap` row (vlm-dlv3p-bn12-sk4-ftap-mcvitb, clip_encoder=None) at crop 64, 5 classes, B = 2, one
        full semi-supervised step with BatchNorm in train mode; the head's buffers are stored after the step.
Case D: one supervised step of B's model with the reference's own ProbOhemCrossEntropy2d; thresh / min_kept chosen as in
        gen_golden_ohem_step.py (thresh in the widest gap of the target-class probabilities, min_kept below the count it
        keeps) so that the relabelling bites; the relabelled map is stored.
Per case: losses, label maps with their tie masks, the norm of every trainable tensor's gradient, the full gradients of
noguidance_ref.GRAD_FULL, input and weight checksums.  The float32 run of the same modules is printed next to each stored
quantity (the noise floor the tests' limits are read against) and its label maps must differ from the float64 run's only
inside the tie budget of golden_util.assert_labels."""
import os
import runpy
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (paths, the mask feeder, the 'tiny' dimensions)
from golden_util import assert_labels, seeded_state, smooth_batch  # noqa: E402
import noguidance_ref as R  # noqa: E402

SEED, LOGIT_GAIN, DSEED = 41, 150.0, 42


def build_reference_unguided(c):
    import model.vlm as ref_vlm  # noqa: registers VLM
    import model.decode_heads.vlg_head  # noqa: registers VLGHead
    import third_party.maskclip.models.backbones.maskclip_vit  # noqa: registers the ViT
    from model.builder import forward_wrapper
    mcfg = runpy.run_path("configs/_base_/models/vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb.py")["model"]
    S = c["S"]
    bb = mcfg["backbone"]
    bb.update(img_size=(S, S), embed_dims=c["embed"], num_layers=c["layers"], num_heads=c["heads"],
              out_indices=c["out_indices"])
    bb.pop("pretrained", None)
    bb["type"] = "MaskClipVisionTransformer"
    mcfg["decode_head"].update(img_size=S, num_classes=21, text_channels=c["text_channels"], up_channels=c["up"],
                               skip_in_channels=(c["embed"], c["embed"]), skip_channels=c["skip"],
                               num_heads=c["dec_heads"], channels=c["channels"], type="VLGHead")
    mcfg.pop("type")
    mcfg.pop("pretrained", None)
    m = ref_vlm.VLM(load_text_embedding=G.TEXT, load_mcc_text_embedding=G.MCC_TEXT, load_pl_text_embedding=G.TEXT,
                    clip_encoder=None, maskclip_class_filter=None, **mcfg)       # experiments.py:197-202
    assert m.clip_encoder is None
    m.disable_dropout, m.fp_rate = True, 0.5
    m.forward = types.MethodType(forward_wrapper, m)
    return m


class Adapter:
    def __init__(s, m):
        s.m = m

    def eval(s):
        s.m.eval()

    def train(s):
        s.m.train()

    def named_parameters(s):
        return s.m.named_parameters()

    def __call__(s, img, need_fp=False, fp_masks=None):
        return s.m(img, need_fp=need_fp)


def main():
    os.chdir(G.REF)
    sys.path.insert(0, G.REF)
    import _ref_shim_dlv3p
    _ref_shim_dlv3p.install()       # (_ref_shim.install() + the decode-head base class the DeepLabV3+ head derives from)
    from oracle import semivl_oracle as O
    import utils.train_utils as ref_tu

    def ref_cwl(loss, conf, ign, conf_mode, conf_thresh):
        return ref_tu.confidence_weighted_loss(loss, conf, ign, dict(conf_mode=conf_mode, conf_thresh=conf_thresh))

    helpers = (ref_tu.cutmix_img_, ref_tu.cutmix_mask, ref_cwl)
    c = dict(G.CONFIGS["tiny"], seed=SEED, logit_gain=LOGIT_GAIN, smooth_inputs=True)
    B, S = c["B"], c["S"]
    batch = smooth_batch(O.synthetic_batch(B, S, 21, seed=1234 + c["seed"]))
    g = torch.Generator().manual_seed(c["seed"] + 100)
    fp_masks = [(torch.rand(2 * B, ch, generator=g) > 0.5).float() for ch in (c["embed"], c["embed"], 512)]
    ref = build_reference_unguided(c)
    sd = seeded_state([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], c["seed"], c["logit_gain"])
    assert not any(k.startswith("clip_encoder.") for k in sd)
    # the confidence gate (gen_golden.py's 'auto'): the middle of the widest gap between two confidences of the float64 run
    torch.set_default_dtype(torch.float64)
    keep = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        ref.double().load_state_dict(sd, strict=True)
        feeder, orig = G.MaskFeeder([m.double() for m in fp_masks]), F.dropout2d
        F.dropout2d = feeder
        try:
            with torch.no_grad():
                _, a0 = R.semivl_step_unguided(Adapter(ref), {k: v.double() if v.is_floating_point() else v for k, v in batch.items()},
                                               0.0, "pixelwise", None, helpers)
        finally:
            F.dropout2d = orig
    finally:
        torch.Tensor.float = keep
        torch.set_default_dtype(torch.float32)
    vals = torch.cat([a0["conf_w"].flatten(), a0["conf_w_other"].flatten()]).sort().values
    lo, hi = vals[int(0.25 * len(vals))], vals[int(0.75 * len(vals))]
    gaps, mid = vals[1:] - vals[:-1], 0.5 * (vals[1:] + vals[:-1])
    gaps = torch.where((mid > lo) & (mid < hi), gaps, torch.zeros_like(gaps))
    j = int(gaps.argmax())
    assert gaps[j].item() >= 2e-4, f"no confidence gap >= 2e-4 in the middle half ({gaps[j].item():.2e})"
    c["conf_thresh"] = round(float(mid[j]), 6)
    print(f"conf_thresh {c['conf_thresh']} (gap {gaps[j].item():.2e})")

    def run(case, f64):
        to = (lambda t: t.double() if t.is_floating_point() else t) if f64 else (lambda t: t)
        keep = torch.Tensor.float
        if f64:
            torch.set_default_dtype(torch.float64)
            torch.Tensor.float = lambda self, *a, **k: self.double()
        try:
            torch.manual_seed(c["seed"])
            ref = build_reference_unguided(c)
            ref.load_state_dict(sd, strict=True)
            assert all(p.dtype == (torch.float64 if f64 else torch.float32) for p in ref.parameters())
            bt = {k: to(v) for k, v in batch.items()}
            if case == "A":
                masks = [to(m) for m in fp_masks]
                feeder, orig = G.MaskFeeder(masks), F.dropout2d
                F.dropout2d = feeder
                try:
                    loss, aux = R.semivl_step_unguided(Adapter(ref), bt, c["conf_thresh"], "pixelwise", masks, helpers)
                finally:
                    F.dropout2d = orig
            else:
                loss, pred = R.supervised_step(Adapter(ref), bt, torch.nn.CrossEntropyLoss(ignore_index=255))
                aux = dict(pred_x=pred)
            loss.backward()
            assert loss.dtype == (torch.float64 if f64 else torch.float32)
            return loss.detach(), aux, R.grads_of(ref)
        finally:
            torch.Tensor.float = keep
            torch.set_default_dtype(torch.float32)

    out = dict(cfg=np.array(repr(dict(c, name="noguidance"))),
               fp_masks=np.concatenate([m.numpy().ravel() for m in fp_masks]).astype(np.uint8),
               state_keys=np.array(list(sd)),
               in_checksum=np.array([sum(v.double().sum().item() for v in batch.values())]),
               w_checksum=np.array([sum(v.double().sum().item() for v in sd.values()),
                                    sum(v.double().abs().sum().item() for v in sd.values())]))
    rel = lambda a, b: ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    for case in ("A", "C"):
        l32, a32, g32 = run(case, False)
        loss, aux, rg = run(case, True)
        assert set(g32) == set(rg) and all(k in rg for k in R.GRAD_FULL)
        pre = case + "/"
        print(f"[{case}] loss float64 {loss.item():.10f}; float32 run |d| {abs(l32.item() - loss.item()):.2e}")
        out[pre + "loss"] = loss.numpy()
        if case == "A":
            for k in ("loss_x", "loss_s1", "loss_s2", "loss_fp"):
                print(f"    {k:8s} {aux[k].item():.10f}  float32 run |d| {abs(a32[k].item() - aux[k].item()):.2e}")
                assert aux[k].item() > 0, k
                out[pre + k] = aux[k].detach().numpy()
            cf = torch.cat((aux["conf_w"].flatten(), aux["conf_w_other"].flatten()))
            margin = (cf - c["conf_thresh"]).abs().min().item()
            print(f"    confidences: closest to the threshold {margin:.2e}; {float((cf >= c['conf_thresh']).double().mean()):.2f} pass")
            assert margin >= 9e-5
            for k, p in (("mask_w", "pred_w"), ("mask_w_other", "pred_w_other")):
                tie = R.label_ties(aux[p], 1e-6 * c["logit_gain"])
                n = assert_labels(a32[k].numpy(), aux[k].numpy(), tie.numpy(), k)
                print(f"    {k}: float32 run differs at {n} pixels, all on ties ({int(tie.sum())} tie pixels)")
                out[pre + k] = aux[k].numpy().astype(np.uint8)
                out[pre + "tie/" + k] = np.packbits(tie.numpy())
        else:
            out[pre + "pred_x_s16"] = aux["pred_x"].detach()[:, :, ::16, ::16].numpy()
            print(f"    pred_x: float32 run max |d| {(a32['pred_x'].double() - aux['pred_x']).abs().max().item():.2e}")
        out[pre + "grad_names"] = np.array(sorted(rg))
        ngap = {k: abs(g32[k].double().norm().item() / rg[k].norm().item() - 1) for k in rg if rg[k].norm() > 1e-6}
        fgap = {k: rel(g32[k], rg[k]) for k in rg if rg[k].norm() > 1e-6}
        # (head.bias' gradient is sum(softmax - onehot) ~ 0: pure cancellation noise, left out of the relative figures)
        print(f"    {len(rg)} grads; float32 run: gradient norms worst rel {max(ngap.values()):.2e} ({max(ngap, key=ngap.get)}), "
              f"full gradients worst rel max {max(fgap.values()):.2e} ({max(fgap, key=fgap.get)})")
        for k in sorted(rg):
            out[pre + "gnorm/" + k] = np.array([rg[k].norm().item(), rg[k].flatten()[0].item(), rg[k].flatten()[-1].item()])
        for k in R.GRAD_FULL:
            out[pre + "grad/" + k] = rg[k].numpy()
    dlv3p_cases(out, helpers, O)
    path = os.path.join(HERE, "semivl_noguidance.npz")
    np.savez_compressed(path, **out)
    print(f"    wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB; semivl_ft.npz: "
          f"{os.path.getsize(os.path.join(HERE, 'semivl_ft.npz')) / 1e6:.2f} MB)")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "semivl_ft.npz"))


def build_reference_dlv3p(crop, nclass):
    import model.vlm as ref_vlm  # noqa: registers VLM
    import model.decode_heads.dlv3p_head  # noqa: registers DLV3PHead
    import third_party.maskclip.models.backbones.maskclip_vit  # noqa: registers the ViT
    from model.builder import forward_wrapper
    mcfg = runpy.run_path("configs/_base_/models/vlm-dlv3p-bn12-sk4-ftap-mcvitb.py")["model"]
    mcfg["backbone"].update(img_size=(crop, crop))
    mcfg["backbone"].pop("pretrained", None)
    mcfg["decode_head"].update(img_size=crop, num_classes=nclass)
    mcfg.pop("type")
    mcfg.pop("pretrained", None)
    m = ref_vlm.VLM(load_text_embedding=G.TEXT, load_mcc_text_embedding=G.MCC_TEXT, load_pl_text_embedding=G.TEXT,
                    clip_encoder=None, maskclip_class_filter=None, **mcfg)
    assert m.clip_encoder is None
    m.disable_dropout, m.fp_rate = True, 0.5
    m.forward = types.MethodType(forward_wrapper, m)
    return m


def widest_gap(vals, lo_q, hi_q, need):
    """The middle of the widest gap between two neighbours of the sorted values inside their [lo_q, hi_q] quantile range."""
    vals = vals.double().sort().values
    lo, hi = vals[int(lo_q * len(vals))], vals[int(hi_q * (len(vals) - 1))]
    gaps, mid = vals[1:] - vals[:-1], 0.5 * (vals[1:] + vals[:-1])
    gaps = torch.where((mid > lo) & (mid < hi), gaps, torch.zeros_like(gaps))
    j = int(gaps.argmax())
    assert gaps[j].item() >= need, f"no gap >= {need} ({gaps[j].item():.2e})"
    return round(float(mid[j]), 6), gaps[j].item()


def dlv3p_cases(out, helpers, O):
    """Cases B (one semi-supervised step) and D (one supervised step with the reference's own ProbOhemCrossEntropy2d) of the
    DeepLabV3+ `ftap` row at crop 64, 5 classes, B = 2, BatchNorm in train mode; the buffers are stored after the step."""
    from third_party.unimatch.util.ohem import ProbOhemCrossEntropy2d
    crop, nclass, B, seed = 64, 5, 2, DSEED
    batch = smooth_batch(O.synthetic_batch(B, crop, nclass, seed=1234 + seed))
    g = torch.Generator().manual_seed(seed + 100)
    fp_masks = [(torch.rand(2 * B, ch, generator=g) > 0.5).float() for ch in (768, 512)]
    ref = build_reference_dlv3p(crop, nclass)
    sd = seeded_state([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], seed)
    assert not any(k.startswith("clip_encoder.") for k in sd)
    del ref

    def run(case, f64, conf_thresh=None, crit_kw=None):
        to = (lambda t: t.double() if t.is_floating_point() else t) if f64 else (lambda t: t)
        keep = torch.Tensor.float
        if f64:
            torch.set_default_dtype(torch.float64)
            torch.Tensor.float = lambda self, *a, **k: self.double()
        try:
            ref = build_reference_dlv3p(crop, nclass)
            ref.load_state_dict(sd, strict=True)
            assert all(p.dtype == (torch.float64 if f64 else torch.float32) for p in ref.parameters())
            bt = {k: to(v) for k, v in batch.items()}
            if case == "B":
                feeder, orig = G.MaskFeeder([to(m) for m in fp_masks]), F.dropout2d
                F.dropout2d = feeder
                try:
                    loss, aux = R.semivl_step_unguided(Adapter(ref), bt, conf_thresh, "pixelwise", None, helpers)
                finally:
                    F.dropout2d = orig
            else:
                crit, seen = None, {}
                if crit_kw is not None:
                    crit = ProbOhemCrossEntropy2d(**crit_kw)
                    crit.criterion.register_forward_pre_hook(lambda m_, args: seen.update(t=args[1].clone()))
                loss, pred = R.supervised_step(Adapter(ref), bt, crit)
                aux = dict(pred_x=pred, mask_x_ohem=seen.get("t"))
            if loss.requires_grad:
                loss.backward()
            bufs = {k: v.detach().clone() for k, v in ref.decode_head.named_buffers()}
            return loss.detach(), aux, R.grads_of(ref), bufs
        finally:
            torch.Tensor.float = keep
            torch.set_default_dtype(torch.float32)

    # the confidence gate of B and the OHEM threshold of D, both from the float64 run's own values
    with torch.no_grad():
        _, a0, _, _ = run("B", True, conf_thresh=0.0)
    conf_thresh, gap = widest_gap(torch.cat([a0["conf_w"].flatten(), a0["conf_w_other"].flatten()]), 0.25, 0.75, 1e-4)
    print(f"[B] conf_thresh {conf_thresh} (gap {gap:.2e})")
    with torch.no_grad():
        _, d0, _, _ = run("D", True)
    px, mx = d0["pred_x"], batch["mask_x"]
    valid = mx != 255
    pt = F.softmax(px, dim=1).gather(1, (mx * valid).unsqueeze(1)).squeeze(1)[valid]
    thresh, gap = widest_gap(pt, 0.05, 0.995, 4e-5)
    min_kept = int((pt <= thresh).sum()) // 2
    crit_kw = dict(ignore_index=255, thresh=thresh, min_kept=min_kept)
    print(f"[D] thresh {thresh} (gap {gap:.2e}), min_kept {min_kept}, valid {len(pt)}")
    out["dlv3p/cfg"] = np.array(repr(dict(crop=crop, nclass=nclass, B=B, seed=seed, conf_thresh=conf_thresh,
                                          criterion=dict(name="OHEM", kwargs=crit_kw))))
    out["dlv3p/fp_masks"] = np.concatenate([m.numpy().ravel() for m in fp_masks]).astype(np.uint8)
    out["dlv3p/state_keys"] = np.array(list(sd))
    out["dlv3p/in_checksum"] = np.array([sum(v.double().sum().item() for v in batch.values())])
    out["dlv3p/w_checksum"] = np.array([sum(v.double().sum().item() for v in sd.values()),
                                        sum(v.double().abs().sum().item() for v in sd.values())])
    rel = lambda a, b: ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    for case in ("B", "D"):
        kw = dict(conf_thresh=conf_thresh) if case == "B" else dict(crit_kw=crit_kw)
        l32, a32, g32, b32 = run(case, False, **kw)
        loss, aux, rg, bufs = run(case, True, **kw)
        assert set(g32) == set(rg) and all(k in rg for k in R.GRAD_FULL_DLV3P)
        pre = case + "/"
        print(f"[{case}] loss float64 {loss.item():.10f}; float32 run |d| {abs(l32.item() - loss.item()):.2e}")
        out[pre + "loss"] = loss.numpy()
        if case == "B":
            for k in ("loss_x", "loss_s1", "loss_s2", "loss_fp"):
                print(f"    {k:8s} {aux[k].item():.10f}  float32 run |d| {abs(a32[k].item() - aux[k].item()):.2e}")
                assert aux[k].item() > 0, k
                out[pre + k] = aux[k].detach().numpy()
            cf = torch.cat((aux["conf_w"].flatten(), aux["conf_w_other"].flatten()))
            print(f"    confidences: closest to the threshold {(cf - conf_thresh).abs().min().item():.2e}; "
                  f"{float((cf >= conf_thresh).double().mean()):.2f} pass")
            for k, p in (("mask_w", "pred_w"), ("mask_w_other", "pred_w_other")):
                tie = R.label_ties(aux[p])
                n = assert_labels(a32[k].numpy(), aux[k].numpy(), tie.numpy(), k)
                print(f"    {k}: float32 run differs at {n} pixels, all on ties ({int(tie.sum())} tie pixels)")
                out[pre + k] = aux[k].numpy().astype(np.uint8)
                out[pre + "tie/" + k] = np.packbits(tie.numpy())
        else:
            kept = int((aux["mask_x_ohem"] != 255).sum())
            assert min_kept < kept < len(pt), (min_kept, kept, len(pt))
            assert torch.equal(aux["mask_x_ohem"], a32["mask_x_ohem"]), "float32 run relabels differently"
            print(f"    OHEM keeps {kept} of {len(pt)} labelled pixels (float32 run: the same map)")
            out[pre + "mask_x_ohem"] = aux["mask_x_ohem"].numpy().astype(np.uint8)
        out[pre + "grad_names"] = np.array(sorted(rg))
        ngap = {k: abs(g32[k].double().norm().item() / rg[k].norm().item() - 1) for k in rg if rg[k].norm() > 1e-6}
        fgap = {k: rel(g32[k], rg[k]) for k in rg if rg[k].norm() > 1e-6}
        print(f"    {len(rg)} grads; float32 run: gradient norms worst rel {max(ngap.values()):.2e} ({max(ngap, key=ngap.get)}), "
              f"full gradients worst rel max {max(fgap.values()):.2e} ({max(fgap, key=fgap.get)})")
        for k in sorted(rg):
            out[pre + "gnorm/" + k] = np.array([rg[k].norm().item(), rg[k].flatten()[0].item(), rg[k].flatten()[-1].item()])
        for k in R.GRAD_FULL_DLV3P:
            out[pre + "grad/" + k] = rg[k].numpy()
        bgap = 0.0
        for k, v in bufs.items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == (2 if case == "B" else 1), (k, int(v))
            else:
                bgap = max(bgap, (b32[k].double() - v).abs().max().item())
            out[pre + "stat/" + k] = v.numpy()
        print(f"    BatchNorm running statistics after the step: float32 run max |d| {bgap:.2e}")


if __name__ == "__main__":
    main()
