"""Golden vectors for the zero-shot MaskCLIP model part (MaskClip2Head + prompt denoising + key smoothing).  Runs ONLY where the
reference tree exists, on the CPU, and calls the reference's OWN code in float64 (and float32, for the noise floor):
`MaskClipHead.refine_output` (maskclip_head.py:129-155), `TransformerEncoderLayer.forward_qkv` (maskclip_vit.py:110-118),
`MaskClip2Head` and `VLM` + `forward_wrapper` at the fixtures' tiny dimensions -- through tests/golden/_ref_shim.py and the
`BaseDecodeHead` stand-in of _ref_shim_dlv3p.py for the un-vendored mmseg / mmcv.  Writes tests/golden/maskclip_refine.npz: data
only (inputs, thresholds, recorded results).

    python tests/golden/gen_golden_maskclip.py

refine/<case>/...   synthetic logits and keys (tests/maskclip_refine_ref.draw_case: every threshold decision >= 1e-3 from its
                    threshold in float64, asserted here) through refine_output; one case drops every class (pd_thresh = 1.5),
                    one holds a NaN logit, one has both refinements off, one each alone.
keys/...            a block input, the block's tensors and forward_qkv's k.
model/...           VLM + MaskClip2Head (embed 64, 3 layers, 21 VOC text rows) on a 80 x 64 input with img_size 64: cosine
                    logits, keys, and for the four threshold pairs the refined token map in float64, the distance of the float32
                    run from it, the label map at input size and its float64 top-2 gap.  Asserted: the same margins, the
                    smoothed-row / dropped-class conditions, and that the float32 run's labels differ from the float64 run's
                    only where the gap is within twice the limit the test applies (4 x that distance), on at most 1 % of the
                    pixels.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

U = 2.0 ** -24
PD, KS = 0.5, 0.7
REFINE_CASES = dict(                 # name -> (B, h, w, N, E, seed, pd_thresh, ks_thresh)
    both=(2, 6, 5, 9, 16, 1, PD, KS), pd_only=(2, 6, 5, 9, 16, 2, PD, 0.0), ks_only=(2, 6, 5, 9, 16, 3, 0.0, KS),
    off=(1, 3, 4, 5, 8, 4, 0.0, 0.0), drop_all=(2, 4, 4, 6, 8, 5, 1.5, KS), nan=(2, 6, 5, 9, 16, 6, PD, KS),
    wide=(1, 8, 8, 21, 32, 7, PD, KS))
MODEL = dict(S=64, B=2, embed=64, layers=3, heads=1, H=80, W=64, seed=0)
PAIRS = ((0.0, 0.0), (PD, 0.0), (0.0, KS), (PD, KS))
TEXT = "configs/_base_/datasets/text_embedding/voc12_wbg_single.npy"


def ref_refine(refine_output, x, k, hw, pd, ks):
    """The reference's refine_output on logits x [B, HW, N] (handed over as its NCHW map) -> [B, N, HW]."""
    B, HW, N = x.shape
    ns = types.SimpleNamespace(pd_thresh=pd, ks_thresh=ks)
    out = refine_output(ns, x.transpose(1, 2).reshape(B, N, *hw).clone(), None if k is None else k.clone())
    return out.reshape(B, N, HW)


def check_conditions(r, pd, ks, what, need_mix=True):
    import maskclip_refine_ref as R
    m = R.margins(r, pd, ks)
    assert min(m) >= R.MARGIN, (what, m)
    if need_mix and pd > 0 and pd <= 1:
        for b in range(r["dropped"].shape[0]):
            d = int(r["dropped"][b].sum())
            assert d >= 1 and r["dropped"].shape[1] - d >= 2, (what, b, d)
    if need_mix and r["selected"] is not None and pd <= 1:
        f = float(r["selected"].double().mean())
        assert 0.1 <= f <= 0.9, (what, f)
    return m


def refine_cases(out, refine_output):
    import maskclip_refine_ref as R
    for name, (B, h, w, N, E, seed, pd, ks) in REFINE_CASES.items():
        x, k = R.draw_case(B, h * w, N, E, seed, pd, ks, nan_at=(0, 3, 1) if name == "nan" else None)
        r = R.refine_ref(x, k, pd, ks)
        m = check_conditions(r, pd, ks, name, need_mix=name not in ("nan", "off"))
        if name == "drop_all":
            assert bool(r["dropped"].all()) and bool(r["selected"].all())
            assert float((r["P"] - 1.0 / N).abs().max()) < 1e-15
        want = ref_refine(refine_output, x.double(), k.double(), (h, w), pd, ks)
        got = r["out"]
        assert torch.equal(torch.isnan(want), torch.isnan(got)), name
        d = float((want - got).abs().nan_to_num(0.0).max())
        assert d <= 1e-12, (name, d)
        print(f"refine/{name}: margins {m[0]:.2e} / {m[1]:.2e}, dropped {r['dropped'].sum(1).tolist()} of {N}, smoothed "
              f"{'-' if r['selected'] is None else round(float(r['selected'].double().mean()), 3)}, restatement |d| {d:.1e}")
        out[f"refine/{name}/x"], out[f"refine/{name}/k"] = x.numpy(), k.numpy()
        out[f"refine/{name}/dims"] = np.array([B, h, w, N, E], dtype=np.int64)
        out[f"refine/{name}/thresh"] = np.array([pd, ks], dtype=np.float64)
        out[f"refine/{name}/out"] = want.numpy()


def keys_case(out, layer_cls):
    g = torch.Generator().manual_seed(11)
    B, T, E = 2, 7, 16
    layer = layer_cls(embed_dims=E, num_heads=2, feedforward_channels=4 * E, norm_cfg=dict(type="LN", eps=1e-6)).double()
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=g).double() * 0.3)
    x = torch.randn(B, T, E, generator=g).double()
    with torch.no_grad():
        k = layer.forward_qkv(x)[1][:, 1:]
    a = layer.attn.attn
    out["keys/x"], out["keys/k"] = x.numpy(), k.numpy()
    for n, t in (("ln_w", layer.norm1.weight), ("ln_b", layer.norm1.bias), ("in_w", a.in_proj_weight), ("in_b", a.in_proj_bias),
                 ("out_w", a.out_proj.weight), ("out_b", a.out_proj.bias)):
        out["keys/" + n] = t.detach().numpy()
    out["keys/eps"] = np.float64(layer.norm1.eps)


def model_image(c):
    g = torch.Generator().manual_seed(100 + c["seed"])
    img = torch.randn(c["B"], 3, c["H"], c["W"], generator=g)
    img = F.avg_pool2d(img, 5, stride=1, padding=2)
    return (img / img.std()).contiguous()


def build_model(c, forward_wrapper, ref_vlm, runpy):
    bb = runpy.run_path("configs/_base_/models/mcvit16.py")["backbone"]
    bb.update(img_size=(c["S"], c["S"]), embed_dims=c["embed"], num_layers=c["layers"], num_heads=c["heads"])
    bb.pop("pretrained", None)
    head = dict(type="MaskClip2Head", img_size=c["S"], in_channels=512, channels=512, num_classes=21, align_corners=False,
                in_index=-1)
    m = ref_vlm.VLM(load_text_embedding=TEXT, load_mcc_text_embedding=TEXT, load_pl_text_embedding=TEXT, clip_encoder=None,
                    maskclip_class_filter=None, backbone=bb, decode_head=head)
    m.disable_dropout, m.fp_rate = True, 0.5
    m.forward = types.MethodType(forward_wrapper, m)
    return m


def run_model(m, img, refine_output, dtype):
    """dict: logits [B, N, hp, wp], keys [B, HW, E], per pair the refined token map [B, N, hp, wp] and the final map."""
    m = m.to(dtype).eval()
    img = img.to(dtype)
    seen = {}
    hook = m.backbone.layers[-1].register_forward_pre_hook(lambda mod, args: seen.__setitem__("x", args[0].detach().clone()))
    with torch.no_grad():
        x = m.extract_feat(img)
        feat = x[0][0][-1]
        logits = m.decode_head.cls_seg(feat, x[1])
        keys = m.backbone.layers[-1].forward_qkv(seen["x"])[1][:, 1:]
        whole = m(img)
    hook.remove()
    B, N, hp, wp = logits.shape
    res = dict(logits=logits, keys=keys)
    for pd, ks in PAIRS:
        with torch.no_grad():
            tok = refine_output(types.SimpleNamespace(pd_thresh=pd, ks_thresh=ks), logits.clone(),
                                keys.clone() if ks > 0 else None)
            fin = F.interpolate(tok, size=(m.decode_head.img_size,) * 2, mode="bilinear", align_corners=False)
            fin = F.interpolate(fin, size=img.shape[2:], mode="bilinear", align_corners=False)
        if pd == 0 and ks == 0:
            assert torch.equal(fin, whole), "the composed path is not forward_wrapper's"
        res[(pd, ks)] = (tok, fin)
    return res


def model_case(out, refine_output, forward_wrapper, ref_vlm, runpy):
    import maskclip_refine_ref as R
    from golden_util import seeded_state
    c = dict(MODEL)
    for seed in range(64):          # the first seed whose float64 run keeps every decision MARGIN away from its threshold
        c["seed"] = seed
        m = build_model(c, forward_wrapper, ref_vlm, runpy)
        shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if k.startswith("backbone.")]
        sd = seeded_state(shapes, 500 + seed)
        m.load_state_dict(sd, strict=False)
        img = model_image(c)
        r64 = run_model(m, img, refine_output, torch.float64)
        B, N, hp, wp = r64["logits"].shape
        xr = r64["logits"].reshape(B, N, hp * wp).transpose(1, 2)
        try:
            for pd, ks in PAIRS[1:]:
                check_conditions(R.refine_ref(xr, r64["keys"], pd, ks), pd, ks, f"model seed {seed} {pd}/{ks}")
        except AssertionError as e:
            print("model: seed", seed, "rejected:", e)
            continue
        break
    else:
        raise AssertionError("no model seed with the margins")
    m32 = build_model(c, forward_wrapper, ref_vlm, runpy)
    m32.load_state_dict(sd, strict=False)
    r32 = run_model(m32, img, refine_output, torch.float32)
    out["model/cfg"] = np.array(repr(c))
    out["model/w_checksum"] = np.array([sum(v.double().sum().item() for v in sd.values()),
                                        sum(v.double().abs().sum().item() for v in sd.values())])
    out["model/img_checksum"] = np.array([img.double().sum().item(), img.double().abs().sum().item()])
    out["model/logits"], out["model/keys"] = r64["logits"].numpy(), r64["keys"].numpy()
    out["model/logits_dist_f32"] = np.float64((r32["logits"].double() - r64["logits"]).abs().max())
    for pd, ks in PAIRS:
        tag = f"model/{pd}_{ks}"
        tok64, fin64 = r64[(pd, ks)]
        tok32, fin32 = r32[(pd, ks)]
        rr = R.refine_ref(xr, r64["keys"] if ks > 0 else None, pd, ks)
        d_re = float((rr["out"].reshape(B, N, hp, wp) - tok64).abs().max())
        assert d_re <= 1e-12, (tag, d_re)
        dist = float((tok32.double() - tok64).abs().max())
        limit = 4.0 * max(dist, U)
        t2 = fin64.topk(2, dim=1).values
        gap = t2[:, 0] - t2[:, 1]
        lab64, lab32 = fin64.argmax(1), fin32.argmax(1)
        excl = gap <= 2.0 * limit
        assert float(excl.double().mean()) <= 0.01, (tag, float(excl.double().mean()))
        assert bool((lab64 == lab32)[~excl].all()), tag
        print(f"{tag}: float32 run {dist:.2e} from float64, limit {limit:.2e}, excluded pixels {int(excl.sum())} of {excl.numel()}, "
              f"labels used {lab64.unique().numel()}, restatement |d| {d_re:.1e}")
        out[tag + "/map"], out[tag + "/dist_f32"] = tok64.numpy(), np.float64(dist)
        out[tag + "/labels"], out[tag + "/gap"] = lab64.numpy().astype(np.uint8), gap.numpy().astype(np.float32)


def main():
    os.chdir(REF)
    sys.path.insert(0, REF)
    import runpy
    import _ref_shim_dlv3p
    _ref_shim_dlv3p.install()
    import model.vlm as ref_vlm  # noqa: registers VLM
    import third_party.maskclip.models.backbones.maskclip_vit as ref_vit  # noqa: registers the ViT
    import third_party.maskclip.models.decode_heads.maskclip2_head  # noqa: registers MaskClip2Head
    from third_party.maskclip.models.decode_heads.maskclip_head import MaskClipHead
    from model.builder import forward_wrapper
    torch.manual_seed(0)
    out = {}
    refine_cases(out, MaskClipHead.refine_output)
    keys_case(out, ref_vit.TransformerEncoderLayer)
    model_case(out, MaskClipHead.refine_output, forward_wrapper, ref_vlm, runpy)
    path = os.path.join(HERE, "maskclip_refine.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 500_000, size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
