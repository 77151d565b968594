"""The two loop bodies the unguided rows of experiment 41 run, restated over ANY model object (plain torch, any dtype):

  semivl_step_unguided   semivl.py:223-328 along its `maskclip_consistency_lambda == 0` branches (:234,262,283,296,309,312,
                         320 are all skipped): no forward_maskclip, no guidance maps, no guidance terms;
  supervised_step        third_party/unimatch/supervised.py:277-289: one train-mode forward and the criterion.

`model(img, need_fp=False, fp_masks=None)` returns logits at input resolution, with need_fp the pair (plain, feature-
perturbed) of the doubled batch, like the reference's forward_wrapper.  `helpers` = (cutmix_img_, cutmix_mask,
confidence_weighted_loss(loss, conf, ign, conf_mode, conf_thresh)): the generator (tests/golden/gen_golden_noguidance.py)
passes the reference's own utils/train_utils.py functions, the tests the restatements below.  Nothing here calls the
product's code."""
import torch
import torch.nn.functional as F

GRAD_FULL_DLV3P = ("decode_head.head.6.weight", "decode_head.head.6.bias", "decode_head.head.4.weight",
                   "decode_head.aspp.b4.gap.2.bias", "backbone.layers.0.attn.attn.out_proj.bias",
                   "backbone.layers.11.attn.attn.out_proj.bias", "backbone.layers.5.attn.attn.in_proj_bias")
GRAD_FULL = ("decode_head.head.weight", "backbone.pos_embed", "backbone.layers.1.attn.attn.out_proj.weight")


def cutmix_img_(img, img_mix, box):  # train_utils.py:19-21
    m = box.unsqueeze(1).expand(img.shape) == 1
    img[m] = img_mix[m]


def cutmix_mask(mask, mask_mix, box):  # train_utils.py:24-27
    out = mask.clone()
    out[box == 1] = mask_mix[box == 1]
    return out


def confidence_weighted_loss(loss, conf_map, ignore_mask, conf_mode, conf_thresh):  # train_utils.py:30-49
    valid = ignore_mask != 255
    sp = dict(dim=(1, 2), keepdim=True)
    if conf_mode == "pixelwise":
        loss = loss * ((conf_map >= conf_thresh) & valid)
        return loss.sum() / valid.sum().item()
    if conf_mode == "pixelratio":
        r = ((conf_map >= conf_thresh) & valid).sum(**sp) / valid.sum(**sp)
        return (loss * r).sum() / valid.sum().item()
    if conf_mode == "pixelavg":
        avg = (conf_map * valid).sum(**sp) / valid.sum(**sp)
        return (loss.sum() * avg).sum() / valid.sum().item()
    raise ValueError(conf_mode)


def guided(cfg):
    """semivl.py:83,158: the reference's own test on the cfg value (missing key = the default [0.1, 0])."""
    return cfg.get("maskclip_consistency_lambda", [0.1, 0]) != 0


def semivl_step_unguided(model, batch, conf_thresh, conf_mode="pixelwise", fp_masks=None, helpers=None):
    """-> (loss, aux).  `batch`: the 12 step tensors (cloned: the CutMix of the images is in place)."""
    mix_img_, mix, cwl = helpers or (cutmix_img_, cutmix_mask, confidence_weighted_loss)
    b = {k: v.clone() for k, v in batch.items()}
    mix_img_(b["img_s1"], b["img_s1_other"], b["mix1"])                                   # :224-225
    mix_img_(b["img_s2"], b["img_s2_other"], b["mix2"])
    with torch.no_grad():                                                                 # :228-232
        model.eval()
        pred_w_other = model(b["img_w_other"]).detach()
        conf_w_other, mask_w_other = pred_w_other.softmax(dim=1).max(dim=1)
    model.train()                                                                         # :243
    preds, preds_fp = model(torch.cat((b["img_x"], b["img_w"])), need_fp=True, fp_masks=fp_masks)   # :245-247
    pred_x, pred_w = preds.chunk(2)
    _, pred_w_fp = preds_fp.chunk(2)
    pred_s1, pred_s2 = model(torch.cat((b["img_s1"], b["img_s2"]))).chunk(2)              # :249
    pred_w = pred_w.detach()                                                              # :251-252
    conf_w, mask_w = pred_w.softmax(dim=1).max(dim=1)
    mw1, mw2 = mix(mask_w, mask_w_other, b["mix1"]), mix(mask_w, mask_w_other, b["mix2"])  # :255-260
    cw1, cw2 = mix(conf_w, conf_w_other, b["mix1"]), mix(conf_w, conf_w_other, b["mix2"])
    ig1 = mix(b["ignore_mask"], b["ignore_mask_other"], b["mix1"])
    ig2 = mix(b["ignore_mask"], b["ignore_mask_other"], b["mix2"])
    ce_none = lambda p, t: F.cross_entropy(p, t, reduction="none")
    loss_x = F.cross_entropy(pred_x, b["mask_x"], ignore_index=255)                      # :268
    loss_s1 = cwl(ce_none(pred_s1, mw1), cw1, ig1, conf_mode, conf_thresh)                # :275-276
    loss_s2 = cwl(ce_none(pred_s2, mw2), cw2, ig2, conf_mode, conf_thresh)                # :288-289
    loss_fp = cwl(ce_none(pred_w_fp, mask_w), conf_w, b["ignore_mask"], conf_mode, conf_thresh)   # :301-302
    loss = (loss_x + loss_s1 * 0.25 + loss_s2 * 0.25 + loss_fp * 0.5) / 2.0               # :319
    aux = dict(loss_x=loss_x, loss_s1=loss_s1, loss_s2=loss_s2, loss_fp=loss_fp, mask_w=mask_w,
               mask_w_other=mask_w_other, conf_w=conf_w, conf_w_other=conf_w_other, pred_x=pred_x, pred_w=pred_w,
               pred_w_other=pred_w_other)
    return loss, aux


def supervised_step(model, batch, criterion=None):
    """supervised.py:268,277-280 -> (loss, pred).  `criterion`: None = nn.CrossEntropyLoss(ignore_index=255) (the 'CELoss'
    of the configs), else a callable (pred, mask) -> loss such as ohem.py's ProbOhemCrossEntropy2d."""
    model.train()
    pred = model(batch["img_x"])
    loss = (criterion or torch.nn.CrossEntropyLoss(ignore_index=255))(pred, batch["mask_x"])
    return loss, pred


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def label_ties(pred, eps=1e-6):
    """Pixels where an argmax over classes sits on a floating-point tie (top-2 logit gap < eps), as golden_util.tie_masks."""
    t = pred.detach().topk(2, dim=1).values
    return (t[:, 0] - t[:, 1]) < eps
