"""GPU: the zero-shot MaskCLIP model through the evaluators.  `evaluate` / `evaluate_report` in mode 'original' on three small
synthetic images give the table counted from the float64 restatement's labels (tests/maskclip_refine_ref.py applied to the
model's own logits and keys, the two bilinear resizes in float64); and the path a user walks -- convert_clip_weights on a
(synthetic) CLIP archive, tools.text_embeddings for an own class list, `tools.eval --save-path none` -- runs end to end."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import evalreport_ref as E
import maskclip_refine_ref as R
import text_ref as T
from golden_util import seeded_state
from test_text_tool_gpu import CLASSES, MERGES, TEMPLATE

pytestmark = pytest.mark.gpu
PD, KS = 0.5, 0.7
U = 2.0 ** -24


def _images(sizes, nclass, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        img = F.avg_pool2d(torch.randn(1, 3, h, w, generator=g), 5, stride=1, padding=2)
        lbl = torch.randint(0, nclass, (1, h // 8 + 1, w // 8 + 1), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
        lbl = lbl[:, :h, :w].contiguous()
        lbl[:, :3] = 255
        out.append(((img / img.std()).contiguous(), lbl, f"JPEGImages/im{i}.png SegmentationClass/im{i}.png"))
    return out


def _restated_labels(model, rec, img, S):
    """(labels [1, H, W], tie mask) of the float64 restatement on the model's own logits and keys.  Tie: the float64 top-2 gap
    of a pixel is within twice the largest end-to-end bound among its classes; the token map's element-wise bounds (P's for an
    unsmoothed row, the product stage's plus sum_j |W_ij| P's for a smoothed one) go through the two bilinear resizes with the
    values (non-negative weights that sum to 1), plus the resizes' own fp32 roundings."""
    B, (hp, wp) = img.shape[0], rec["hw"]
    HW = hp * wp
    x, k = rec["x"].cpu().view(B, HW, -1), rec["k"].cpu().view(B, HW, -1)
    N, Ed = x.shape[2], k.shape[2]
    r = R.refine_ref(x, k, PD, KS)
    P64, pb = R.p_bound(x, r["dropped"])
    mag = k.double().abs() @ (R.s_ref(k.reshape(B * HW, Ed), B, HW)[0].view(B, Ed, 1) * (k.double().abs().transpose(1, 2) @ P64.view(B, HW, N)))
    bound = R.SECOND * R.gamma(HW + Ed + 4) * mag + r["W"].abs() @ pb.view(B, HW, N)
    bound = torch.where(r["selected"][:, :, None], bound, pb.view(B, HW, N)).transpose(1, 2).reshape(B, N, hp, wp)

    def resize(t):
        t = F.interpolate(t, size=(S, S), mode="bilinear", align_corners=False)
        return F.interpolate(t, size=img.shape[2:], mode="bilinear", align_corners=False)

    fin = resize(r["out"].view(B, N, hp, wp))
    fin_bound = resize(bound) + 16 * U * fin.abs()          # the same non-negative weights carry the bounds; + the resizes' roundings
    t2 = fin.topk(2, dim=1).values
    return fin.argmax(1), (t2[:, 0] - t2[:, 1]) <= 2 * fin_bound.max(1).values


def test_evaluators_count_the_restatements_labels(dev):
    from semivl_amd.evaluate import evaluate
    from semivl_amd.report import evaluate_report
    from test_maskclip_model_gpu import build, spy
    torch.manual_seed(21)
    S, K = 64, 21
    model = build(S, 64, 3, 1, pd_thresh=PD, ks_thresh=KS)
    # the golden fixture's seeded O(1) weights (tests/golden/gen_golden_maskclip.py): a trunc_normal(0.02) initialisation gives
    # near-uniform probabilities, whose label decisions mostly sit inside the comparison's own tie band
    model.load_state_dict(seeded_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 500), strict=True)
    model.to(dev).eval()
    data = _images([(64, 80), (80, 64), (64, 64)], K, 3)
    rec = spy(model)
    labels, ties = [], []
    with torch.no_grad():
        for img, _, _ in data:
            out = model(img.to(dev))
            want, tie = _restated_labels(model, rec, img, S)
            got = out.argmax(1).cpu()
            assert bool((got == want)[~tie].all())
            labels.append(torch.where(tie, got, want))            # on a tie either label is the restatement's
            ties.append(tie)
    assert sum(int(t.sum()) for t in ties) <= 0.01 * sum(t.numel() for t in ties)
    cfg = dict(crop_size=S, nclass=K, eval_report=dict(metrics=["mIoU", "mAcc"]))
    rep = evaluate_report(model, data, "original", cfg)
    want = sum(E.confusion_ref(l.to(dev), m.to(dev), K).cpu().numpy() for l, (_, m, _) in zip(labels, data))
    assert np.array_equal(rep.table.reshape(-1), want.reshape(-1))
    assert int(rep.table.sum()) == sum(int((m != 255).sum()) for _, m, _ in data)
    miou, iou = evaluate(model, data, "original", cfg)
    assert rep.miou == miou and np.array_equal(rep.iou_class, iou) and 0.0 <= miou <= 100.0
    assert len(set(torch.cat([l.reshape(-1) for l in labels]).tolist())) >= 3          # not one constant map


def _visual_state(width, layers, grid, seed):
    """A CLIP visual tower's tensors under OpenAI's names (ViT, patch 16), seeded; fp16 like the archive."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)
    sd = {"visual.class_embedding": rn(width, sc=0.05), "visual.positional_embedding": rn(grid * grid + 1, width, sc=0.05),
          "visual.conv1.weight": rn(width, 3, 16, 16, sc=(3 * 256) ** -0.5), "visual.proj": rn(width, 512, sc=width ** -0.5)}
    for ln in ("ln_pre", "ln_post"):
        sd[f"visual.{ln}.weight"], sd[f"visual.{ln}.bias"] = 1 + rn(width, sc=0.1), rn(width, sc=0.02)
    for i in range(layers):
        p = f"visual.transformer.resblocks.{i}."
        sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = rn(3 * width, width, sc=width ** -0.5), rn(3 * width, sc=0.02)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = rn(width, width, sc=width ** -0.5), rn(width, sc=0.02)
        for ln in ("ln_1", "ln_2"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = 1 + rn(width, sc=0.1), rn(width, sc=0.02)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = rn(4 * width, width, sc=width ** -0.5), rn(4 * width, sc=0.02)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = rn(width, 4 * width, sc=(4 * width) ** -0.5), rn(width, sc=0.02)
    return {k: v.half() for k, v in sd.items()}


def test_eval_tool_from_archive_to_metric_table(dev, tmp_path, capsys):
    """convert_clip_weights --backbone --text, tools.text_embeddings, tools.eval --save-path none: zero-shot, nothing trained."""
    import yaml
    from PIL import Image
    from semivl_amd.model.builder import builtin_model_cfg
    from semivl_amd.model.maskclip_head import MaskClip2Head
    from semivl_amd.tools import convert_clip_weights, text_embeddings
    from semivl_amd.tools.eval import main
    d = tmp_path
    S, width, layers = 64, 64, 2
    sd = T.seeded_clip_text_state(9, 512 + len(MERGES) + 2, 128, 2, 512, 31, dtype=torch.float16)
    sd.update(_visual_state(width, layers, S // 16, 7))
    sd["logit_scale"] = torch.tensor(4.6052)
    torch.save(sd, d / "clip.pt")
    (d / "merges.txt").write_text("#version: synthetic\n" + "\n".join(" ".join(m) for m in MERGES) + "\n", encoding="utf-8")
    (d / "classes.json").write_text(json.dumps(CLASSES))
    convert_clip_weights.main(["--src", str(d / "clip.pt"), "--backbone", "--text", "--out-dir", str(d / "pretrained")])
    text_embeddings.main(["--clip", str(d / "pretrained" / "clip_ViT16_text_encoder.pth"), "--bpe", str(d / "merges.txt"),
                          "--classes", str(d / "classes.json"), "--variant", "single", "--out", str(d / "mine.npy"),
                          "--template", TEMPLATE])
    K = len(CLASSES)
    root = d / "data"
    os.makedirs(root / "JPEGImages")
    os.makedirs(root / "SegmentationClass")
    ids = []
    for i, (img, lbl, id_) in enumerate(_images([(64, 80), (72, 64), (64, 64)], K, 9)):
        u8 = ((img[0] * 60 + 128).clamp(0, 255)).permute(1, 2, 0).to(torch.uint8).numpy()
        Image.fromarray(u8).save(root / "JPEGImages" / f"im{i}.png")
        Image.fromarray(lbl[0].to(torch.uint8).numpy()).save(root / "SegmentationClass" / f"im{i}.png")
        ids.append(id_)
    (d / "val.txt").write_text("\n".join(ids) + "\n")
    m = copy.deepcopy(builtin_model_cfg("vlm-maskclip2-mcvitb"))["model"]
    m["backbone"].update(img_size=(S, S), embed_dims=width, num_layers=layers, num_heads=1)
    m["decode_head"].update(img_size=S, num_classes=K, pd_thresh=PD, ks_thresh=KS)
    cfg = dict(dataset="pascal", data_root=str(root), val_id_path=str(d / "val.txt"), nclass=K, crop_size=S,
               model="mmseg.vlm-maskclip2-mcvitb", text_embedding_files=dict(text=str(d / "mine.npy")), disable_dropout=True,
               fp_rate=0.5, eval_report=dict(metrics=["mIoU", "mAcc"]),
               model_args=dict(backbone=m["backbone"], decode_head=m["decode_head"],
                               pretrained=str(d / "pretrained" / "clip2mmseg_ViT16_clip_backbone.pth")))
    with open(d / "cfg.yaml", "w") as f:
        yaml.dump(cfg, f)
    rep = main(["--config", str(d / "cfg.yaml"), "--save-path", "none", "--pred-path", str(d / "pred"),
                "--report-json", str(d / "report.json")])
    out = capsys.readouterr().out
    assert "NO CHECKPOINT SPECIFIED" in out and "***** Evaluation original *****" in out and rep.format_table() in out
    assert rep.K == K and int(rep.table.sum()) > 0 and 0.0 <= rep.miou <= 100.0
    assert sorted(os.listdir(d / "pred")) == ["im0.png", "im1.png", "im2.png"]
    rj = json.load(open(d / "report.json"))
    assert rj["images"] == 3 and rj["nclass"] == K and rj["eval_mode"] == "original"
    # the model the tool built: the converted weights, not a random init
    from semivl_amd.model.builder import build_model
    model = build_model(dict(cfg, clip_encoder=None))
    assert isinstance(model.decode_head, MaskClip2Head) and model.decode_head.ks_thresh == KS
    want = sd["visual.transformer.resblocks.1.attn.in_proj_weight"].float()
    assert torch.equal(model.backbone.layers[1].attn.attn.in_proj_weight.detach(), want)
    assert torch.equal(model.backbone.proj.weight.detach()[:, :, 0, 0], sd["visual.proj"].float().t())
