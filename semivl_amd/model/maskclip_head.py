"""`MaskClip2Head` (third_party/maskclip/models/decode_heads/maskclip2_head.py): the parameter-free zero-shot head.  It scores
the backbone's unit-norm dense embedding against the text rows (cosine logits, maskclip2_head.py:29-33) and resizes the map to
(img_size, img_size) (maskclip2_head.py:23).  No training: forward_train raises in the reference, the training steps refuse here.

Extension (not in the reference's MaskClip2Head, taken from its MaskClipHead.refine_output, maskclip_head.py:129-155):
`pd_thresh` (prompt denoising) and `ks_thresh` (key smoothing) refine the token-resolution map in eval mode before the resize
(ops.mc_refine).  Both default to 0 = off; the head then returns the reference's logits.
"""
import torch.nn as nn

from .. import ops


def _thresh(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0:
        raise ValueError(f"MaskClip2Head: {name} must be a real number >= 0, got {v!r}")
    return float(v)


class MaskClip2Head(nn.Module):
    """Constructor signature: the reference's config keys (mmseg `BaseDecodeHead` arguments included; `in_channels`, `channels`
    and the rest describe nothing this head builds and are accepted, not used)."""

    trainable = False    # the training steps: there is nothing to train (maskclip2_head.py:35-36)

    def __init__(self, img_size, in_channels, channels, num_classes, align_corners=False, in_index=-1, pd_thresh=0.,
                 ks_thresh=0., dropout_ratio=0, conv_cfg=None, norm_cfg=None, act_cfg=None, input_transform=None,
                 loss_decode=None, ignore_index=255, sampler=None, init_cfg=None, type=None):
        super().__init__()
        self.image_size = self.img_size = img_size
        self.in_channels, self.channels, self.num_classes = in_channels, channels, num_classes
        self.align_corners, self.in_index = align_corners, in_index
        self.pd_thresh, self.ks_thresh = _thresh("pd_thresh", pd_thresh), _thresh("ks_thresh", ks_thresh)
        self.conv_seg = None
        self.load_text_embedding = None      # set by VLM like the reference

    def wants_keys(self):
        """The last block's keys are only read by key smoothing, which only runs in eval mode (maskclip_head.py:118)."""
        return self.ks_thresh > 0 and not self.training

    def forward_tokens(self, x, k, B, hw):
        """x [B * HW, N] cosine logits (token rows), k [B * HW, E] keys or None -> the map [B, N, h, w] at token resolution:
        refined in eval mode, x itself (as class planes) in train mode or with both thresholds 0."""
        HW = hw[0] * hw[1]
        pd, ks = (0.0, 0.0) if self.training else (self.pd_thresh, self.ks_thresh)
        with ops.prof_scope("head"):
            return ops.mc_refine(x, k, B, HW, pd, ks).view(B, x.shape[1], hw[0], hw[1])

    def forward_train(self, *args, **kw):
        raise RuntimeError("MaskClip is not trainable. Try MaskClip+ instead.")
