"""Import shim used ONLY by tests/golden/gen_golden_dlv3p.py (where the reference tree exists): `_ref_shim.install()` plus
a restatement of the part of mmseg 0.24's `BaseDecodeHead.__init__` the reference's DLV3PHead relies on -- the attributes
it reads (`in_channels`, `num_classes`, `align_corners`) and the two sub-modules the base class creates (`conv_seg`, which
DLV3PHead sets to None, and `dropout`, None at dropout_ratio 0), so the head's `state_dict` keys come out as under mmseg.
Nothing here is reference source; nothing here travels into the product."""
import sys

import torch.nn as nn

import _ref_shim


class BaseDecodeHead(_ref_shim.BaseModule):
    def __init__(self, in_channels, channels, *, num_classes, dropout_ratio=0.1, conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type="ReLU"), in_index=-1, input_transform=None, loss_decode=None, ignore_index=255,
                 sampler=None, align_corners=False, init_cfg=None):
        super().__init__(init_cfg)
        assert input_transform is None
        self.in_channels, self.channels, self.num_classes = in_channels, channels, num_classes
        self.dropout_ratio, self.conv_cfg, self.norm_cfg, self.act_cfg = dropout_ratio, conv_cfg, norm_cfg, act_cfg
        self.in_index, self.ignore_index, self.align_corners = in_index, ignore_index, align_corners
        self.conv_seg = nn.Conv2d(channels, num_classes, kernel_size=1)
        self.dropout = nn.Dropout2d(dropout_ratio) if dropout_ratio > 0 else None


def install():
    _ref_shim.install()
    sys.modules["mmseg.models.decode_heads.decode_head"].BaseDecodeHead = BaseDecodeHead
