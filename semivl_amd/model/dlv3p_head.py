"""DeepLabV3+ decoder on the CLIP ViT: the reference's `DLV3PHead` (model/decode_heads/dlv3p_head.py) with UniMatch's
`ASPPModule` (third_party/unimatch/model/semseg/deeplabv3plus.py:76-126), the head of the ablation rows
`vlm-dlv3p-bn12-sk4-{ft,ftap}-mcvitb` of experiment 41.

    c1 = block-4 tokens [n, HW, 768], c4 = CLIP embedding map [n, HW, 512], both at crop / 16
    aspp(c4):  1x1 | 3x3 d6 | 3x3 d12 | 3x3 d18 | global pool -> 1x1, each 512 -> 64 + BN + ReLU; concat 320 -> 1x1 -> 64 + BN + ReLU
    c1_proj:   1x1 768 -> 48 + BN + ReLU
    head:      cat(c1, c4) 112 -> 3x3 256 + BN + ReLU -> 3x3 256 + BN + ReLU -> 1x1 N (bias)

The modules below are parameter containers with the reference's `state_dict` keys (`aspp.b0.0.weight`,
`aspp.b4.gap.2.running_mean`, `head.6.bias`, ...), initialised by their torch constructors like the reference
(`init_cfg=None`).  Everything runs channels-last on the library, token layout [n * HW, C]: 1x1 convs as GEMMs, 3x3 convs
through ops.conv_fwd / conv_dgrad / conv_wgrad (which kernel serves a dilation at a map size is their business), BatchNorm
through `svl_bn_*` with batch statistics reduced in double (all-reduced through resnet._sync_sums = SyncBN when
torch.distributed is initialised), the pooled branch through `svl_gap_tokens_*` / `svl_bcast_rows_*`.  Branch outputs are
written straight into their channel slice of the concat slabs (BatchNorm's apply pass takes a destination stride), so no
concat copies exist.  The pooled branch's resize of a 1 x 1 map (align_corners=True) is a broadcast; the resize of c4 to
c1's size (dlv3p_head.py:56) is the identity for a ViT, where both maps are at crop / 16.

One `autograd.Function` spans the head: forward saves what BatchNorm backward needs (pre-normalisation tensors, mean,
invstd; the ReLU masks are re-derived from them), backward is written by hand and sends weight gradients to the parameters'
`main_grad` sinks when present, as model/resnet.py does.

BatchNorm couples the samples of a decoded batch, so -- unlike the VLG head -- nothing of a batch may be skipped: the
feature-perturbed copies of `forward_wrapper`'s need_fp pass (builder.py:78-89) are all decoded, and backward runs on the
whole batch (rows whose dlogits are zero still carry gradient through the statistics terms)."""
import torch
import torch.nn as nn

from .. import gradsync, ops
from .resnet import _sync_sums
from .vlg_head import _GradCollector


def _conv_bn_relu(cin, cout, k, dil=1):
    return nn.Sequential(nn.Conv2d(cin, cout, k, padding=0 if k == 1 else dil, dilation=dil, bias=False),
                         nn.BatchNorm2d(cout), nn.ReLU(True))


class ASPPPooling(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.gap = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout),
                                 nn.ReLU(True))


class ASPPModule(nn.Module):
    def __init__(self, cin, dilations):
        super().__init__()
        cout = cin // 8
        self.b0 = _conv_bn_relu(cin, cout, 1)
        self.b1, self.b2, self.b3 = (_conv_bn_relu(cin, cout, 3, d) for d in dilations)
        self.b4 = ASPPPooling(cin, cout)
        self.project = _conv_bn_relu(5 * cout, cout, 1)


# ------------------------------------------------------------------------------------------------ units
def _bn(z, bn, training, out=None, sv=None):
    """relu(batchnorm(z [rows, C])) written to `out` (a [rows, C] tensor or a channel slice of a wider slab)."""
    C = z.shape[1]
    if training:
        sums = ops.bn_stats(z, C)
        world = _sync_sums(sums)
        count = z.shape[0] * world
        mean, invstd = ops.bn_finalize(sums, count, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
        bn.num_batches_tracked += 1
    else:
        mean, invstd, count = bn.running_mean, ops.bn_eval_invstd(bn.running_var, bn.eps), z.shape[0]
    y = ops.bn_apply(z, C, mean, invstd, bn.weight, bn.bias, relu=True, out=out)
    if sv is not None:
        sv.update(z=z, mean=mean, invstd=invstd, count=count)
    return y


def _bn_bwd(dy, bn, sv, gc):
    """dz from dy (a tensor or a channel slice of a wider gradient slab); the ReLU mask is re-derived from z."""
    z = sv["z"]
    C = z.shape[1]
    sums = ops.bn_bwd_reduce(dy, z, None, C, sv["mean"], sv["invstd"], remask=(bn.weight, bn.bias))
    gc.put_tensor(bn.bias, sums[0].float())      # this rank's sums: the data-parallel mean is the reducer's job
    gc.put_tensor(bn.weight, sums[1].float())
    _sync_sums(sums)
    return ops.bn_bwd_apply(dy, z, None, C, sv["mean"], sv["invstd"], bn.weight, sums, sv["count"], remask_beta=bn.bias)


def _w2d(conv):
    return conv.weight.view(conv.weight.shape[0], conv.weight.shape[1])


def _conv3(x, ldx, geo, conv, sv):
    imgs, H, W = geo
    Co, Ci = conv.weight.shape[:2]
    d = conv.dilation[0]
    wf, wd = ops.pack_conv_w(conv.weight)
    if sv is not None:
        sv["wd"] = wd
    return ops.conv_fwd(x, ldx, imgs, H, W, Ci, wf, Co, 3, 3, d, d)


def _conv3_bwd(dz, x, ldx, geo, conv, sv, gc, dx=None):
    """Weight gradient to the collector; the input gradient written to (dx None) or accumulated onto dx [rows, Ci]."""
    imgs, H, W = geo
    Co, Ci = conv.weight.shape[:2]
    d = conv.dilation[0]
    dwf = ops.conv_wgrad(dz, Co, x, ldx, imgs, H, W, Ci, Co, 3, 3, d, d)
    gc.put_tensor(conv.weight, ops.unpack_conv_wgrad(dwf, Co, Ci, 3, 3))
    if dx is None:
        return ops.conv_dgrad(dz, Co, imgs, H, W, Co, sv["wd"], Ci, 3, 3, d, d)
    return ops.conv_dgrad(dz, Co, imgs, H, W, Co, sv["wd"], Ci, 3, 3, d, d, out=dx, ldo=Ci, accumulate=True)


def _double(f, mask, scale):
    """[n, HW, C] -> ([n' * HW, C], n'): with a channel mask the batch is followed by its F.dropout2d copy
    (cat((f, dropout2d(f))), builder.py:78-89)."""
    n, HW, C = f.shape
    f2 = f.contiguous().view(n * HW, C)
    if mask is None:
        return f2, n
    out = ops.empty(2 * n * HW, C, device=f.device)
    ops.eltwise(4, f2.view(-1), None, out=out.view(-1)[:n * HW * C])
    ops.chanmask(f2, mask.contiguous(), scale, HW, out=out[n * HW:])
    return out, 2 * n


def _double_bwd(d, mask, scale, n, HW):
    if mask is None:
        return d.view(n, HW, -1)
    C = d.shape[1]
    lo = d[:n * HW]
    hi = ops.chanmask(d[n * HW:], mask.contiguous(), scale, HW)
    return ops.add(lo.reshape(-1), hi.view(-1)).view(n, HW, C)


# ------------------------------------------------------------------------------------------------ forward / backward
def _head_forward(m, c1, c4, hw, fp_masks, fp_scale, out_size, sv):
    """c1 [n, HW, 768], c4 [n, HW, 512] -> logits [n', N, S, S]."""
    H, W = hw
    HW = H * W
    tr = m.training
    S = (lambda: {}) if sv is not None else (lambda: None)
    mk1, mk4 = fp_masks if fp_masks is not None else (None, None)
    x1, n2 = _double(c1, mk1, fp_scale)
    x4, _ = _double(c4, mk4, fp_scale)
    R, geo = n2 * HW, (n2, H, W)
    a = m.aspp
    Cb = a.b0[0].weight.shape[0]                       # 64
    Cc1 = m.c1_proj[0].weight.shape[0]                 # 48
    s = {k: S() for k in ("b0", "b1", "b2", "b3", "b4", "pj", "c1", "h0", "h3", "k1", "k2", "k3", "q0", "q3")}
    cat = ops.empty(R, 5 * Cb, device=x4.device)
    _bn(ops.linear(x4, _w2d(a.b0[0])), a.b0[1], tr, out=cat[:, :Cb], sv=s["b0"])
    for i, (br, ks) in enumerate(((a.b1, "k1"), (a.b2, "k2"), (a.b3, "k3")), 1):
        _bn(_conv3(x4, x4.shape[1], geo, br[0], s[ks]), br[1], tr, out=cat[:, i * Cb:(i + 1) * Cb], sv=s[f"b{i}"])
    pool = ops.gap_tokens_fwd(x4, n2, HW)                                        # AdaptiveAvgPool2d(1)
    yp = _bn(ops.linear(pool, _w2d(a.b4.gap[1])), a.b4.gap[2], tr, sv=s["b4"])   # BatchNorm over n' rows
    ops.bcast_rows_fwd(yp, n2, HW, cat, 4 * Cb)                                  # 1 x 1 -> H x W resize + concat
    fuse = ops.empty(R, Cc1 + Cb, device=x4.device)                              # cat([c1, c4], 1)
    _bn(ops.linear(x1, _w2d(m.c1_proj[0])), m.c1_proj[1], tr, out=fuse[:, :Cc1], sv=s["c1"])
    _bn(ops.linear(cat, _w2d(a.project[0])), a.project[1], tr, out=fuse[:, Cc1:], sv=s["pj"])
    h1 = _bn(_conv3(fuse, fuse.shape[1], geo, m.head[0], s["q0"]), m.head[1], tr, sv=s["h0"])
    h2 = _bn(_conv3(h1, h1.shape[1], geo, m.head[3], s["q3"]), m.head[4], tr, sv=s["h3"])
    N = m.head[6].weight.shape[0]
    lt = ops.linear(h2, _w2d(m.head[6]), bias=m.head[6].bias)                    # [R, N]
    lg = ops.permute4(lt, (n2, N, HW, 1), (HW * N, 1, N, 1)).view(n2, N, H, W)
    if tuple(out_size) != (H, W):
        lg = ops.bilinear_planes_fwd(lg, H, W, m.align_corners, out_size[0], out_size[1])
    if sv is not None:
        sv.update(s=s, x1=x1, x4=x4, cat=cat, fuse=fuse, h1=h1, h2=h2, pool=pool, geo=geo, n=c1.shape[0],
                  masks=(mk1, mk4), fp_scale=fp_scale, out_size=tuple(out_size), N=N)
    return lg


def _head_backward(m, dlogits, sv, gc, need_dc1, need_dc4):
    s, geo = sv["s"], sv["geo"]
    n2, H, W = geo
    HW, N = H * W, sv["N"]
    a = m.aspp
    Cb, Cc1 = a.b0[0].weight.shape[0], m.c1_proj[0].weight.shape[0]
    dlg = dlogits.contiguous()
    if sv["out_size"] != (H, W):
        dlg = ops.bilinear_planes_bwd(dlg, H, W, m.align_corners, sv["out_size"][0], sv["out_size"][1])
    dl = ops.permute4(dlg, (n2, HW, N, 1), (N * HW, 1, HW, 1)).view(n2 * HW, N)
    # head.6 (1x1, bias)
    gc.put_tensor(m.head[6].weight, ops.matmul_tn(dl, sv["h2"]))
    gc.put_tensor(m.head[6].bias, ops.colsum(dl))
    d = ops.matmul_nn(dl, _w2d(m.head[6]))
    # head.3/4, head.0/1
    d = _conv3_bwd(_bn_bwd(d, m.head[4], s["h3"], gc), sv["h1"], sv["h1"].shape[1], geo, m.head[3], s["q3"], gc)
    dfuse = _conv3_bwd(_bn_bwd(d, m.head[1], s["h0"], gc), sv["fuse"], sv["fuse"].shape[1], geo, m.head[0], s["q0"], gc)
    # c1_proj
    dz = _bn_bwd(dfuse[:, :Cc1], m.c1_proj[1], s["c1"], gc)
    gc.put_tensor(m.c1_proj[0].weight, ops.matmul_tn(dz, sv["x1"]))
    dx1 = ops.matmul_nn(dz, _w2d(m.c1_proj[0])) if need_dc1 else None
    # aspp.project
    dz = _bn_bwd(dfuse[:, Cc1:], a.project[1], s["pj"], gc)
    gc.put_tensor(a.project[0].weight, ops.matmul_tn(dz, sv["cat"]))
    dcat = ops.matmul_nn(dz, _w2d(a.project[0]))
    # branches: the input gradients of all five accumulate in dx4 (the 1x1 branch writes it, the others add)
    x4 = sv["x4"]
    dz = _bn_bwd(dcat[:, :Cb], a.b0[1], s["b0"], gc)
    gc.put_tensor(a.b0[0].weight, ops.matmul_tn(dz, x4))
    dx4 = ops.matmul_nn(dz, _w2d(a.b0[0])) if need_dc4 else None
    for i, (br, ks) in enumerate(((a.b1, "k1"), (a.b2, "k2"), (a.b3, "k3")), 1):
        dz = _bn_bwd(dcat[:, i * Cb:(i + 1) * Cb], br[1], s[f"b{i}"], gc)
        if need_dc4:
            _conv3_bwd(dz, x4, x4.shape[1], geo, br[0], s[ks], gc, dx=dx4)
        else:
            dwf = ops.conv_wgrad(dz, Cb, x4, x4.shape[1], n2, H, W, x4.shape[1], Cb, 3, 3, br[0].dilation[0], br[0].dilation[0])
            gc.put_tensor(br[0].weight, ops.unpack_conv_wgrad(dwf, Cb, x4.shape[1], 3, 3))
    dyp = ops.bcast_rows_bwd(dcat, 4 * Cb, Cb, n2, HW)
    dz = _bn_bwd(dyp, a.b4.gap[2], s["b4"], gc)
    gc.put_tensor(a.b4.gap[1].weight, ops.matmul_tn(dz, sv["pool"]))
    if need_dc4:
        ops.gap_tokens_bwd(ops.matmul_nn(dz, _w2d(a.b4.gap[1])), n2, HW, dx=dx4, accumulate=True)
    n, (mk1, mk4) = sv["n"], sv["masks"]
    return (_double_bwd(dx1, mk1, sv["fp_scale"], n, HW) if need_dc1 else None,
            _double_bwd(dx4, mk4, sv["fp_scale"], n, HW) if need_dc4 else None)


class _DLV3PFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, m, hw, fp_masks, fp_scale, out_size, c1, c4, *params):
        sv = {}
        with ops.prof_scope("head"):
            out = _head_forward(m, c1, c4, hw, fp_masks, fp_scale, out_size, sv)
        ctx.m, ctx.sv, ctx.params = m, sv, params
        ctx.need = (ctx.needs_input_grad[5], ctx.needs_input_grad[6])
        gradsync.expect(params)
        return out

    @staticmethod
    def backward(ctx, dlogits):
        m, sv = ctx.m, ctx.sv
        gc = _GradCollector()
        with ops.prof_scope("head"):
            dc1, dc4 = _head_backward(m, dlogits, sv, gc, *ctx.need)
        ctx.sv = None
        gradsync.ready(ctx.params)
        return (None, None, None, None, None, dc1, dc4) + tuple(gc.out.get(id(p)) for p in ctx.params)


class DLV3PHead(nn.Module):
    """Constructor signature: the reference's config keys (mmseg `BaseDecodeHead` arguments included; `channels`,
    `in_index`, `dropout_ratio=0` and `norm_cfg` describe what the reference builds anyway and are checked, not used)."""

    has_batchnorm = True     # the training step: batch statistics couple the samples of a decode, running statistics order the passes

    def __init__(self, c1_in_channels, c1_channels, dilations, img_size, in_channels, num_classes, channels=256,
                 in_index=-1, dropout_ratio=0, norm_cfg=None, align_corners=False, init_cfg=None, loss_decode=None,
                 type=None):
        super().__init__()
        if dropout_ratio:
            raise NotImplementedError("DLV3PHead (HIP): dropout_ratio != 0 (the reference's configs set 0)")
        if norm_cfg is not None and norm_cfg.get("type") not in ("SyncBN", "BN"):
            raise NotImplementedError(f"DLV3PHead (HIP): norm_cfg {norm_cfg!r}")
        if len(tuple(dilations)) != 3 or in_channels % 32 or c1_channels % 4 or c1_in_channels % 4:
            raise NotImplementedError("DLV3PHead (HIP): three dilations; in_channels % 32 == 0, c1 channels % 4 == 0")
        self.image_size, self.num_classes, self.align_corners = img_size, num_classes, align_corners
        self.in_channels, self.channels, self.in_index = in_channels, channels, in_index
        self.aspp = ASPPModule(in_channels, tuple(dilations))
        self.c1_proj = _conv_bn_relu(c1_in_channels, c1_channels, 1)
        fuse = in_channels // 8 + c1_channels
        self.head = nn.Sequential(nn.Conv2d(fuse, 256, 3, padding=1, bias=False), nn.BatchNorm2d(256), nn.ReLU(True),
                                  nn.Conv2d(256, 256, 3, padding=1, bias=False), nn.BatchNorm2d(256), nn.ReLU(True),
                                  nn.Conv2d(256, num_classes, 1, bias=True))
        self.conv_seg = None
        self.load_text_embedding = None      # set by VLM like the reference; this head never reads the text embedding
        # attributes the training step sets on a decode head (the VLG head's memory plan): accepted, unused
        self._bwd_ranges = self._live_class_images = self._remat_step = None
        self.remat = self.chunk_class_images = self.act_limit_bytes = None

    def forward_tokens(self, feats, text=None, hw=None, fp_masks=None, fp_rate=0.5, out_size=None, **unused):
        """feats = [c1 [n, HW, 768], c4 [n, HW, 512]] on the grid `hw`.  fp_masks: None, or two {0,1} masks [n, C_i]: the
        batch is doubled with its channel-dropped copy (builder.py:78-89) and ALL of it is decoded -- with batch statistics
        every sample enters every mean and variance.  Returns logits [n', N, *out_size] (default: image_size^2)."""
        c1, c4 = feats
        out_size = tuple(out_size or (self.image_size, self.image_size))
        scale = 1.0 / (1.0 - fp_rate)
        params = [p for p in self.parameters() if p.requires_grad]
        if torch.is_grad_enabled() and (bool(params) or c1.requires_grad or c4.requires_grad):
            if not self.training:
                raise NotImplementedError("DLV3PHead (HIP): backward through eval-mode BatchNorm is not implemented")
            return _DLV3PFn.apply(self, tuple(hw), fp_masks, scale, out_size, c1, c4, *params)
        with ops.prof_scope("head"):
            return _head_forward(self, c1, c4, tuple(hw), fp_masks, scale, out_size, None)

    def forward(self, inputs, force_output_pred_masks=False):
        """Reference signature (dlv3p_head.py:48-65): inputs = [[[c1, c4], global], text, conv] with
        force_output_pred_masks, else [c1, c4]; NCHW maps."""
        if force_output_pred_masks:
            inputs = inputs[0][0]
        assert len(inputs) == 2
        toks = []
        for f in inputs:
            b, c, h, w = f.shape
            toks.append(f.permute(0, 2, 3, 1).contiguous().view(b, h * w, c))
        assert inputs[0].shape[-2:] == inputs[1].shape[-2:], "c1 and c4 on different grids (not a ViT pyramid)"
        size = (self.image_size, self.image_size) if force_output_pred_masks else (h, w)
        x = self.forward_tokens(toks, None, (h, w), out_size=size)
        return {"pred_masks": x} if force_output_pred_masks else x
