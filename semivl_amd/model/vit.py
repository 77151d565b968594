"""CLIP ViT-B/16 dense encoder in MaskCLIP form on the HIP kernel library.

Mirror of `MaskClipVisionTransformer` / `TransformerEncoderLayer`
(/root/reference third_party/maskclip/models/backbones/maskclip_vit.py:29-144,147-603) for the configurations on
the SemiVL hot path (pre_norm, final_norm, return_clip_embed, return_qkv=True), with the
same constructor kwargs and the same `state_dict` key schema.  LoRA adapters (`lora_layers`,
model/backbone/lora.py) run as MERGED weights: with lora_dropout == 0 the adapter is linear in the projection's own input,
so a block with adapters runs the same kernels on W + s * B @ A (ops.lora_merge) and its adapters' gradients are projected
out of the projection's weight gradient (ops.lora_wgrad).  Deep visual prompts (`num_prompt_tokens` = P) put P rows between
the class token and the patch tokens of every block's input (ops.prompt_rows_fwd) and take them out of its outputs again;
their gradient is the batch sum of the block's input gradient on those rows (ops.prompt_rows_bwd).  Stochastic depth
(`drop_path_rate`) scales a block's residual branches per sample (ops.droppath_add / ops.droppath_scale) at the sites
DROP_PATH_SITES; a block with rate 0 and every eval-mode forward launch what they launch without the option.

The whole forward AND backward of the encoder is hand-scheduled over libsemivl_hip.so (one autograd.Function for
the region): tokens stay in [B*T, C] row-major, attention/FFN/LN backward are explicit kernel sequences, weight
gradients are written straight into the parameters' `main_grad` arena views when present.
Work that cannot change results is skipped (SURVEY App. C "algorithmic"): the v-path re-uses the block's own
in-proj, out_proj is applied to v only, and the last block's x-path is skipped unless the global embedding is
requested.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import gradsync, ops


# ------------------------------------------------------------------------------------------------ parameter holders
class _MHAParams(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dims, dims))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * dims))
        self.out_proj = nn.Linear(dims, dims)
        # nn.MultiheadAttention._reset_parameters (the decoder's transformer layers keep this init; the ViT's
        # init_weights overrides it)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.)


class _AttnParams(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.attn = _MHAParams(dims)


class _FFNParams(nn.Module):
    def __init__(self, dims, hidden):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(dims, hidden), nn.Identity(), nn.Identity()),
                                    nn.Linear(hidden, dims), nn.Identity())


class _LoRAParams(nn.Module):
    """model/backbone/lora.py:21-57: a_<t> / b_<t> (bias-free Linears, a before b, q k v o) for each t in `targets`;
    kaiming_uniform_(a=sqrt(5)) for a_*, zeros for b_*."""

    def __init__(self, dim, r, scaling=1., targets="qkvo"):
        super().__init__()
        self.dim, self.r, self.scaling, self.targets = dim, r, float(scaling), targets
        for t in "qkvo":
            if t in targets:
                setattr(self, "a_" + t, nn.Linear(dim, r, bias=False))
                setattr(self, "b_" + t, nn.Linear(r, dim, bias=False))
        self.reset_parameters()

    def reset_parameters(self):
        for t in "qkvo":
            if t in self.targets:
                nn.init.kaiming_uniform_(getattr(self, "a_" + t).weight, a=math.sqrt(5))
                nn.init.zeros_(getattr(self, "b_" + t).weight)

    def pair(self, t):
        """(A [r, E], B [E, r]) of target t, or None"""
        if t not in self.targets:
            return None
        return getattr(self, "a_" + t).weight, getattr(self, "b_" + t).weight


class TransformerEncoderLayer(nn.Module):
    """Parameter container with the reference's names: ln1, attn.attn.{in_proj_*,out_proj}, [lora.{a,b}_{q,k,v,o}], ln2,
    ffn.layers.{0.0,1} (registered in the reference's order, maskclip_vit.py:73-100)."""

    def __init__(self, embed_dims, num_heads, feedforward_channels, eps=1e-5, lora=None):
        super().__init__()
        self.embed_dims, self.num_heads, self.eps = embed_dims, num_heads, eps
        self.ln1 = nn.LayerNorm(embed_dims, eps=eps)
        self.attn = _AttnParams(embed_dims)
        self.lora = _LoRAParams(embed_dims, **lora) if lora is not None else None
        self.ln2 = nn.LayerNorm(embed_dims, eps=eps)
        self.ffn = _FFNParams(embed_dims, feedforward_channels)

    def plist(self):
        a, f = self.attn.attn, self.ffn.layers
        return dict(ln1w=self.ln1.weight, ln1b=self.ln1.bias, win=a.in_proj_weight, bin=a.in_proj_bias,
                    wout=a.out_proj.weight, bout=a.out_proj.bias, ln2w=self.ln2.weight, ln2b=self.ln2.bias,
                    w1=f[0][0].weight, b1=f[0][0].bias, w2=f[1].weight, b2=f[1].bias)

    def merged_plist(self):
        """plist() of a block with adapters: `win` / `wout` are the effective weights W + s * B @ A (plain tensors, not
        parameters: built once per encoder call, kept by that call's backward).  The q | k | v row blocks of in_proj merge
        in one launch; a block without a target is copied."""
        lo, a, p = self.lora, self.attn.attn, self.plist()
        pairs = [lo.pair(t) for t in "qkv"]
        with torch.no_grad():
            if any(pr is not None for pr in pairs):
                p["win"] = ops.lora_merge(a.in_proj_weight, pairs, lo.scaling)
            if "o" in lo.targets:
                p["wout"] = ops.lora_merge(a.out_proj.weight, [lo.pair("o")], lo.scaling)
        return p


class _PatchEmbedParams(nn.Module):
    def __init__(self, cin, dims, patch, bias):
        super().__init__()
        self.projection = nn.Conv2d(cin, dims, patch, stride=patch, bias=bias)


# ------------------------------------------------------------------------------------------------ grad sinks
def sink_grad(param, grad_fn, shape=None):
    """Accumulate a gradient for `param`: into its `main_grad` arena view if it has one (returns None so autograd does
    not touch it), else return the tensor to autograd.  `grad_fn(out, accumulate)` writes / accumulates the grad."""
    mg = getattr(param, "main_grad", None)
    if mg is not None:
        grad_fn(mg, True)
        return None
    out = ops.empty(*param.shape, device=param.device)
    grad_fn(out, False)
    return out


# ------------------------------------------------------------------------------------------------ block forward / backward
DROP_PATH_SITES = ("attn", "ffn", "ffn_v")   # x + dp(out_proj(attention)), x2 + dp(FFN(ln2 x2)), vo + dp(FFN(ln2 vo))


def block_forward(x, p, heads, eps, Bn, T, want_v, skip_x, save, dp=None, k_out=None):
    """x [Bn*T, E] -> (x_out or None, v or None).  `save` is a dict to stash what backward needs (or None).
    `k_out`: None, or a list that receives the block's MaskCLIP keys out_proj(in_proj_k(ln1 x)) [Bn*T, E] (forward_qkv,
    maskclip_vit.py:110-118: both biases, no residual): two E x E GEMMs on the ln1 output the block forms anyway.
    `dp`: None, or the block's live stochastic-depth sites: dict(keep=1 - p_i, <site>=mask [Bn] fp32 ...) over DROP_PATH_SITES.
    At a live site the branch's GEMM runs without its residual operand and ops.droppath_add forms identity + (mask_b / keep) *
    branch in place in the branch's buffer.
    Under the packed-planes GEMM path (ops.planes_eligible) every A operand is produced directly in that format: both
    LayerNorms, the FFN-1 epilogue and the fused attention kernel emit planes (ln2's output and gelu(h) exist ONLY as
    planes, the attention output too in gradient-free passes); the v slice of qkv takes the generic split pass."""
    E = x.shape[1]
    D = E // heads
    pp = ops.planes_eligible(x.shape[0], E, E)
    if pp:   # y1 in fp32 is only read by the in_proj weight gradient
        y1, st1, y1a = ops.layernorm_fwd(x, p["ln1w"], p["ln1b"], eps, planes=True, want_y=save is not None)
    else:
        y1, st1 = ops.layernorm_fwd(x, p["ln1w"], p["ln1b"], eps)
        y1a = y1
    if skip_x:
        vproj = ops.linear(y1a, p["win"][2 * E:], p["bin"][2 * E:])
        qkv = None
    else:
        qkv = ops.linear(y1a, p["win"], p["bin"])
        vproj = qkv[:, 2 * E:]
    if k_out is not None:
        kproj = ops.linear(y1a, p["win"][E:2 * E], p["bin"][E:2 * E])
        k_out.append(ops.linear(ops.split_planes(kproj) if pp else kproj, p["wout"], p["bout"]))
    v = None
    if save is not None:
        save.update(x=x, y1=y1, st1=st1, qkv=qkv, vproj=vproj, want_v=want_v, skip_x=skip_x, eps=eps,
                    y1_amax=y1a.amax if pp else None,     # (the maximum of y1 as packed: the in_proj weight gradient's B operand)
                    dp=dp)
    dp = dp or {}

    def ffn(pre, want_pre, mask=None):
        """pre + FFN(LN2(pre)); returns (out, ln2 stats, saved pre-activation or None).  `mask`: the site's drop-path draws."""
        if pp:
            _, st2_, y2a = ops.layernorm_fwd(pre, p["ln2w"], p["ln2b"], eps, planes=True, want_y=False)
        else:
            y2a, st2_ = ops.layernorm_fwd(pre, p["ln2w"], p["ln2b"], eps)
        h_pre_ = ops.empty(pre.shape[0], p["w1"].shape[0], device=x.device) if want_pre else None
        h_ = ops.linear(y2a, p["w1"], p["b1"], act=ops.ACT_GELU, preact=h_pre_, planes_only=True)   # only feeds FFN-2
        if mask is not None:
            return ops.droppath_add(ops.linear(h_, p["w2"], p["b2"]), pre, mask, dp["keep"], Bn, T), st2_, h_pre_
        return ops.linear(h_, p["w2"], p["b2"], resid=pre), st2_, h_pre_

    if want_v:
        vo = ops.linear(ops.split_planes(vproj) if pp else vproj, p["wout"], p["bout"], resid=x)  # out_proj(v) + x   (maskclip_vit.py:115-117)
        v, st2v, hv_pre = ffn(vo, save is not None, dp.get("ffn_v"))
        if save is not None:
            save.update(vo=vo, st2v=st2v, hv_pre=hv_pre)
    xo = None
    if not skip_x:
        o_p = None
        if D == 64 and pp and ops.attention_planes_ok():
            # the kernel's epilogue emits the output as planes (the out-projection's A operand); its fp32 copy is only
            # kept for backward (dsum, out_proj weight gradient)
            # (a pass that saves for backward also keeps the packed Q | K | V operand sets: the backward then packs dO alone)
            o, P, o_p, *sets = ops.attention_fwd(qkv, Bn, T, heads, want_lse=save is not None, planes=True,
                                                 want_out=save is not None, keep_sets=save is not None)
        elif D == 64:
            o, P, *sets = ops.attention_fwd(qkv, Bn, T, heads, want_lse=save is not None, keep_sets=save is not None)  # P := log-sum-exp rows
        else:  # generic head dim: batched-GEMM attention with materialised probabilities
            o, P = ops.vit_attention_fwd(qkv, Bn, T, heads, D)
            sets = []
        o_a = o_p if o_p is not None else (ops.split_planes(o) if pp else o)
        if dp.get("attn") is not None:
            x2 = ops.droppath_add(ops.linear(o_a, p["wout"], p["bout"]), x, dp["attn"], dp["keep"], Bn, T)
        else:
            x2 = ops.linear(o_a, p["wout"], p["bout"], resid=x)
        xo, st2, h_pre = ffn(x2, save is not None, dp.get("ffn"))
        if save is not None:
            save.update(o=o, P=P, x2=x2, st2=st2, h_pre=h_pre, sets=sets[0] if sets else None)
    return xo, v


FFN_LN_KEYS = ("ln1w", "ln1b", "ln2w", "ln2b", "w1", "b1", "w2", "b2")


def block_backward(dxo, dv, p, s, heads, Bn, T, want=frozenset(), dxo_p=None):
    """Returns (dx_in, dx_in planes or None, grads dict).  The attention projections' pieces are always collected (the
    `ftap` recipes train them, vlm.py:66-67); `want` names the FFN / LayerNorm tensors (plist keys, FFN_LN_KEYS) that
    train too (freeze_backbone=False or a wider exclude_keys): only their weight-gradient pieces are produced.
    `dxo_p`: dxo as packed planes when the block above already produced them (its LN1 backward).
    At a live stochastic-depth site (s["dp"]) everything below the site takes (mask_b / keep) * d out (ops.droppath_scale): the
    input-gradient GEMMs, the weight-gradient pieces, the bias sums and the LayerNorm backward's dy; the identity path (dx_add=,
    dx_res) takes d out as it is."""
    x, y1 = s["x"], s["y1"]
    E = x.shape[1]
    D = E // heads
    pp = ops.planes_eligible(x.shape[0], E, E)
    g = {}
    dx_res = None
    dqkv = dqkv_p = dqkv_amax = None     # dqkv_amax: the maximum the pack pass found, valid while dqkv stays as packed
    wout_parts = []  # (dy, input) pairs contributing to out_proj wgrad
    need_h = "w1" in want or "b1" in want
    dp = s.get("dp") or {}

    def ffn_ln_bwd(dout, dout_p, pre_ln_in, st2, h_pre, mask=None):
        """-> (d pre_ln_in, the same as planes or None).  `mask`: the site's drop-path draws (the branch sees the scaled dout)."""
        res = dout      # the identity path's share
        if mask is not None:
            dout = ops.droppath_scale(dout, mask, dp["keep"], Bn, T)
            dout_p = ops.split_planes(dout) if pp else None     # (planes of the unscaled gradient do not describe it)
        # (dout W2) * GELU'(h_pre), one pass; with frozen FFN-1 weights its only consumer is the next GEMM (bf16 planes)
        a_ = dout_p if dout_p is not None else dout
        dhp = ops.matmul_nn(a_, p["w2"], dact=ops.ACT_MUL_DGELU, z=h_pre, planes_only=not need_h)
        dy2 = ops.matmul_nn(dhp, p["w1"])
        # weight-gradient pieces: gelu(h_pre) and LN2(pre_ln_in) are B-operand producers of the weight-gradient GEMMs
        # (recomputed while staging from the saved pre-activation / LayerNorm statistics, never materialised)
        if "w2" in want:
            g.setdefault("w2", []).append(("gelu", dout, h_pre))
        if "b2" in want:
            g.setdefault("b2", []).append(("sum", dout))
        if "w1" in want:
            g.setdefault("w1", []).append(("ln", dhp, pre_ln_in, st2))
        if "b1" in want:
            g.setdefault("b1", []).append(("sum", dhp))
        if "ln2w" in want or "ln2b" in want:
            r_ = ops.layernorm_bwd(dy2, pre_ln_in, st2, p["ln2w"], dx_add=res, want_wgrad=True, planes=pp)
            g.setdefault("ln2w", []).append(("add", r_[1]))
            g.setdefault("ln2b", []).append(("add", r_[2]))
            return r_[0], (r_[3] if pp else None)
        if pp:
            return ops.layernorm_bwd(dy2, pre_ln_in, st2, p["ln2w"], dx_add=res, planes=True)
        return ops.layernorm_bwd(dy2, pre_ln_in, st2, p["ln2w"], dx_add=res), None

    if not s["skip_x"] and dxo is not None:
        dx2, dx2p = ffn_ln_bwd(dxo, dxo_p, s["x2"], s["st2"], s["h_pre"], dp.get("ffn"))
        dbr, dbrp = dx2, dx2p       # d out_proj(attention): the scaled gradient at a live site
        if dp.get("attn") is not None:
            dbr = ops.droppath_scale(dx2, dp["attn"], dp["keep"], Bn, T)
            dbrp = ops.split_planes(dbr) if pp else None
        do = ops.matmul_nn(dbrp if dbrp is not None else dbr, p["wout"])
        wout_parts.append((dbr, s["o"]))
        if D == 64 and pp and ops.attention_planes_ok() and not (s["want_v"] and dv is not None):
            # dqkv also as planes (in_proj's input-gradient GEMM), from the two kernels' epilogues
            dqkv, dqkv_p = ops.attention_bwd(do, s["qkv"], s["o"], s["P"], Bn, T, heads, planes=True, sets=s.get("sets"))
            dqkv_amax = dqkv_p.amax
        elif D == 64:
            dqkv = ops.attention_bwd(do, s["qkv"], s["o"], s["P"], Bn, T, heads, sets=s.get("sets"))
        else:
            dqkv = ops.vit_attention_bwd(do, s["qkv"], s["P"], Bn, T, heads, D)
        dx_res = dx2
    dvproj = None
    if s["want_v"] and dv is not None:
        dvo, dvop = ffn_ln_bwd(dv, None, s["vo"], s["st2v"], s["hv_pre"], dp.get("ffn_v"))
        dvproj = ops.matmul_nn(dvop if dvop is not None else dvo, p["wout"])
        wout_parts.append((dvo, s["vproj"]))
        dx_res = dvo if dx_res is None else ops.add(dx_res, dvo)
    if dqkv is not None and dvproj is not None:
        rows = dqkv.shape[0]
        ops.copy2d(dvproj, 0, rows, 0, E, dqkv, 2 * E, rows, 0, 3 * E, rows, E, accumulate=True)
        dvproj = dqkv_amax = None        # (dqkv is written here: a maximum found before no longer describes it)
    g["wout_parts"] = wout_parts
    if dqkv is not None:
        g["in_full"] = (dqkv, y1, dqkv_amax, s.get("y1_amax"))
        dy1 = ops.matmul_nn(dqkv_p if dqkv_p is not None else dqkv, p["win"])
    elif dvproj is not None:
        g["in_v"] = (dvproj, y1)
        dy1 = ops.matmul_nn(dvproj, p["win"][2 * E:])
    else:
        return dx_res, None, g
    if "ln1w" in want or "ln1b" in want:
        r_ = ops.layernorm_bwd(dy1, x, s["st1"], p["ln1w"], dx_add=dx_res, want_wgrad=True, planes=pp)
        g["ln1w"], g["ln1b"] = [("add", r_[1])], [("add", r_[2])]
        return r_[0], (r_[3] if pp else None), g
    if pp:   # the block below consumes dx_in as the A operand of its d FFN-2 GEMM
        dx_in, dx_in_p = ops.layernorm_bwd(dy1, x, s["st1"], p["ln1w"], dx_add=dx_res, planes=True)
        return dx_in, dx_in_p, g
    return ops.layernorm_bwd(dy1, x, s["st1"], p["ln1w"], dx_add=dx_res), None, g


def ffn_ln_wgrads(p, g):
    """Write the FFN / LayerNorm weight grads of one block from the pieces block_backward collected (x path and v path
    summed).  Returns a dict plist key -> tensor|None (None when written into main_grad)."""
    out = {}
    for key, parts in g.items():
        if key not in FFN_LN_KEYS:
            continue

        def fn(dst, acc, parts=parts):
            for j, part in enumerate(parts):
                a_ = acc or j > 0
                if part[0] == "gelu":
                    ops.matmul_tn_gelu(part[1], part[2], out=dst, accumulate=a_)
                elif part[0] == "ln":
                    ops.matmul_tn_ln(part[1], part[2], part[3], p["ln2w"], p["ln2b"], out=dst, accumulate=a_)
                elif part[0] == "sum":
                    ops.colsum(part[1], out=dst, accumulate=a_)
                elif a_:
                    ops.add(dst, part[1], out=dst)
                else:
                    ops.eltwise(4, part[1], None, out=dst)
        out[key] = sink_grad(p[key], fn)
    return out


def attn_wgrads(p_mod, g, E):
    """Write the attention-projection weight grads of one block from the pieces collected by block_backward.
    Returns a dict name -> tensor|None (None when written into main_grad)."""
    a = p_mod.attn.attn
    out = {}
    if p_mod.lora is not None:
        return _lora_attn_wgrads(p_mod, g, E)
    # a projection whose weight and bias are both frozen launches nothing (a prompts-only recipe: no weight-gradient GEMM,
    # column sum or slab reduction for the blocks at all)
    train_out = a.out_proj.weight.requires_grad or a.out_proj.bias.requires_grad
    train_in = a.in_proj_weight.requires_grad or a.in_proj_bias.requires_grad

    def wout_fn(dst, acc):
        first = not acc
        for dy, xin in g["wout_parts"]:
            ops.matmul_tn(dy, xin, out=dst, accumulate=not first)
            first = False

    def bout_fn(dst, acc):
        first = not acc
        for dy, _ in g["wout_parts"]:
            ops.colsum(dy, out=dst, accumulate=not first)
            first = False

    if g["wout_parts"] and train_out:
        out["wout"] = sink_grad(a.out_proj.weight, wout_fn)
        out["bout"] = sink_grad(a.out_proj.bias, bout_fn)
    else:
        out["wout"] = out["bout"] = None
    if not train_in:
        out["win"] = out["bin"] = None
    elif "in_full" in g:
        dqkv, y1, dq_amax, y1_amax = g["in_full"]
        out["win"] = sink_grad(a.in_proj_weight, lambda dst, acc: ops.matmul_tn(dqkv, y1, out=dst, accumulate=acc,
                                                                                a_amax=dq_amax, b_amax=y1_amax))
        out["bin"] = sink_grad(a.in_proj_bias, lambda dst, acc: ops.colsum(dqkv, out=dst, accumulate=acc))
    elif "in_v" in g:
        dvp, y1 = g["in_v"]

        def win_fn(dst, acc):
            if not acc:
                ops.fill(dst, 0.0)
            ops.matmul_tn(dvp, y1, out=dst[2 * E:], accumulate=acc)

        def bin_fn(dst, acc):
            if not acc:
                ops.fill(dst, 0.0)
            ops.colsum(dvp, out=dst[2 * E:], accumulate=acc)

        out["win"] = sink_grad(a.in_proj_weight, win_fn)
        out["bin"] = sink_grad(a.in_proj_bias, bin_fn)
    else:
        out["win"] = out["bin"] = None
    return out


def _lora_attn_wgrads(p_mod, g, E):
    """attn_wgrads for a block with adapters.  Each projection's weight gradient OF THIS BACKWARD CALL ALONE goes to a
    scratch matrix dW_eff (never main_grad: the step runs the encoder backward twice and main_grad then holds both);
    ops.lora_wgrad folds it into the adapters' sinks (dB = s dW_eff A^T, dA = s B^T dW_eff), and a base projection that
    trains too adds the same scratch to its own sink.  A frozen base projection's sink is not touched.  out["lora"]:
    id(adapter tensor) -> tensor|None (a v-only block: v and o; its q and k adapters get zeros, like the q | k rows of its
    in_proj)."""
    a, lo = p_mod.attn.attn, p_mod.lora
    out = dict(win=None, bin=None, wout=None, bout=None, lora={})

    def adapters(t, dW):
        pr = lo.pair(t)
        if pr is None or not (pr[0].requires_grad or pr[1].requires_grad):
            return
        dst = []
        for prm in pr:
            mg = getattr(prm, "main_grad", None)
            dst.append((mg, True) if mg is not None else (ops.empty(*prm.shape, device=prm.device), False))
        ops.lora_wgrad(dW, pr[0].detach(), pr[1].detach(), lo.scaling, out_b=dst[1][0], out_a=dst[0][0],
                       accumulate_b=dst[1][1], accumulate_a=dst[0][1])
        for prm, (t_, acc) in zip(pr, dst):
            if prm.requires_grad:
                out["lora"][id(prm)] = None if acc else t_

    def base(prm, dW, row0=0):
        """dW (rows [row0, row0 + dW.shape[0]) of prm's gradient, zero elsewhere) into prm's sink"""
        mg = getattr(prm, "main_grad", None)
        if mg is not None:
            dst = mg[row0:row0 + dW.shape[0]]
            ops.add(dst, dW, out=dst)
            return None
        if dW.shape[0] == prm.shape[0]:
            return dW
        full = ops.zeros(*prm.shape, device=prm.device)
        ops.eltwise(4, dW, None, out=full[row0:row0 + dW.shape[0]])
        return full

    if g["wout_parts"]:
        dWo = ops.empty(E, E, device=a.out_proj.weight.device)
        for j, (dy, xin) in enumerate(g["wout_parts"]):
            ops.matmul_tn(dy, xin, out=dWo, accumulate=j > 0)
        adapters("o", dWo)
        if a.out_proj.weight.requires_grad:
            out["wout"] = base(a.out_proj.weight, dWo)
        if a.out_proj.bias.requires_grad:
            def bout_fn(dst, acc):
                for j, (dy, _) in enumerate(g["wout_parts"]):
                    ops.colsum(dy, out=dst, accumulate=acc or j > 0)
            out["bout"] = sink_grad(a.out_proj.bias, bout_fn)
    if "in_full" in g:
        dqkv, y1, dq_amax, y1_amax = g["in_full"]
        dWin = ops.matmul_tn(dqkv, y1, a_amax=dq_amax, b_amax=y1_amax)
        for i, t in enumerate("qkv"):
            adapters(t, dWin[i * E:(i + 1) * E])
        if a.in_proj_weight.requires_grad:
            out["win"] = base(a.in_proj_weight, dWin)
        if a.in_proj_bias.requires_grad:
            out["bin"] = sink_grad(a.in_proj_bias, lambda dst, acc: ops.colsum(dqkv, out=dst, accumulate=acc))
    elif "in_v" in g:
        dvp, y1 = g["in_v"]
        dWv = ops.matmul_tn(dvp, y1)
        adapters("v", dWv)
        for t in "qk":      # the reference's v path adds their (unused) rows too: all-zero gradients, not absent ones
            for prm in lo.pair(t) or ():
                if prm.requires_grad and getattr(prm, "main_grad", None) is None:
                    out["lora"][id(prm)] = ops.zeros(*prm.shape, device=prm.device)
        if a.in_proj_weight.requires_grad:
            out["win"] = base(a.in_proj_weight, dWv, 2 * E)
        if a.in_proj_bias.requires_grad:
            def bin_fn(dst, acc):
                if not acc:
                    ops.fill(dst, 0.0)
                ops.colsum(dvp, out=dst[2 * E:], accumulate=acc)
            out["bin"] = sink_grad(a.in_proj_bias, bin_fn)
    return out


# ------------------------------------------------------------------------------------------------ encoder
class MaskClipVisionTransformer(nn.Module):
    def __init__(self, img_size=224, patch_size=16, patch_bias=True, in_channels=3, embed_dims=768, num_layers=12,
                 num_heads=12, mlp_ratio=4, out_indices=-1, qkv_bias=True, drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., with_cls_token=True, output_cls_token=False, norm_cfg=dict(type='LN'),
                 act_cfg=dict(type='GELU'), patch_norm=False, pre_norm=False, final_norm=False, return_qkv=False,
                 return_clip_embed=False, skip_last_attn=False, interpolate_mode='bicubic', num_fcs=2,
                 norm_eval=False, with_cp=False, pretrained=None, num_prompt_tokens=None, lora_layers=[], lora_r=4,
                 lora_scaling=1, lora_dropout=0, lora_targets='qkvo', init_cfg=None, type=None,
                 allow_random_init=False):
        super().__init__()
        if isinstance(img_size, int):
            img_size = (img_size, img_size)
        unsupported = dict(patch_bias=patch_bias, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate,
                           patch_norm=patch_norm, skip_last_attn=skip_last_attn,
                           output_cls_token=output_cls_token,
                           lora_dropout=lora_dropout if len(lora_layers) else 0)   # (the one part of LoRA that does not merge)
        bad = {k: v for k, v in unsupported.items() if v not in (False, 0, 0.0, None, [])}
        if bad or not (pre_norm and final_norm and return_clip_embed and with_cls_token and qkv_bias):
            raise NotImplementedError(f"MaskClipVisionTransformer (HIP): only the SemiVL hot-path configuration is "
                                      f"implemented (off-path options: {bad}; of the regularisers drop_path_rate is "
                                      f"implemented, drop_rate, attn_drop_rate and lora_dropout are not)")
        if isinstance(drop_path_rate, bool) or not isinstance(drop_path_rate, (int, float)) or not 0 <= drop_path_rate < 1:
            raise ValueError(f"drop_path_rate must be a number in [0, 1), got {drop_path_rate!r}")
        assert act_cfg.get("type") == "GELU" and norm_cfg.get("type") == "LN" and interpolate_mode == "bicubic"
        self.img_size, self.patch_size = tuple(img_size), patch_size
        self.embed_dims, self.num_layers, self.num_heads = embed_dims, num_layers, num_heads
        self.eps = norm_cfg.get("eps", 1e-5)
        self.pretrained = pretrained
        self.allow_random_init = allow_random_init   # benchmarks / tests without the CLIP file (build_model cfg key)
        self.patch_embed = _PatchEmbedParams(in_channels, embed_dims, patch_size, False)
        npatch = (img_size[0] // patch_size) * (img_size[1] // patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dims))
        self.pos_embed = nn.Parameter(torch.zeros(1, npatch + 1, embed_dims))
        if out_indices is None:
            self.out_indices = [num_layers]
        elif isinstance(out_indices, int):
            self.out_indices = [num_layers - 1 if out_indices == -1 else out_indices]
        else:
            self.out_indices = list(out_indices)
        lora = dict(r=lora_r, scaling=lora_scaling, targets=lora_targets)
        self.layers = nn.ModuleList([TransformerEncoderLayer(embed_dims, num_heads, mlp_ratio * embed_dims, self.eps,
                                                             lora=lora if i in lora_layers else None)
                                     for i in range(num_layers)])
        self.ln0 = nn.LayerNorm(embed_dims, eps=self.eps)
        self.ln1 = nn.LayerNorm(embed_dims, eps=self.eps)
        self.proj = nn.Conv2d(embed_dims, 512, 1, bias=False)
        # which blocks run the v-path (maskclip_vit.py:341-355)
        self.return_qkv = [False] * num_layers
        rq = return_qkv if isinstance(return_qkv, (list, tuple)) else [return_qkv] * len(self.out_indices)
        for j, o in enumerate(self.out_indices):
            if o < num_layers:
                self.return_qkv[o] = bool(rq[j])
        self.return_qkv[num_layers - 1] = True
        for o in self.out_indices:
            if o < num_layers and not self.return_qkv[o]:
                raise NotImplementedError("out_indices without return_qkv is off the SemiVL path")
        # deep visual prompts (maskclip_vit.py:359-368).  prompt_norm is never called by the reference's forward: its two
        # tensors are state_dict entries that never receive a gradient (_trainable, optim._trainable).
        self.num_prompt_tokens = num_prompt_tokens
        self.disable_dropout = True         # build_model: cfg['disable_dropout'] (prompt_dropout is live in train mode only when False)
        self.prompt_mask_hook = None        # tests: callable (layer, B) -> {0, 1} mask [B, P, E] (or None) in place of ops.bernoulli
        if num_prompt_tokens is not None:
            if not isinstance(num_prompt_tokens, int) or num_prompt_tokens < 1:
                raise ValueError(f"num_prompt_tokens must be a positive int or None, got {num_prompt_tokens!r}")
            val = math.sqrt(6. / float(3 * patch_size * patch_size + embed_dims))
            self.deep_prompt_embeddings = nn.Parameter(torch.zeros(num_layers, num_prompt_tokens, embed_dims))
            nn.init.uniform_(self.deep_prompt_embeddings.data, -val, val)
            self.prompt_proj = nn.Linear(embed_dims, embed_dims)
            nn.init.kaiming_normal_(self.prompt_proj.weight, a=0, mode="fan_out")
            self.prompt_norm = nn.LayerNorm(embed_dims, eps=1e-6)
            self.prompt_dropout = nn.Dropout(0.1)
        # stochastic depth (maskclip_vit.py:299-312): block i drops its residual branches per sample with rate dpr[i].  Live
        # whenever the module is in train mode and dpr[i] > 0, whatever disable_dropout says (the reference's wrapper does
        # not reach the DropPath of this ViT's blocks).
        self.drop_path_rate = float(drop_path_rate)
        # (host values in fp32, also when the model is built under a meta device or another default dtype)
        self.dpr = [x.item() for x in torch.linspace(0, drop_path_rate, num_layers, dtype=torch.float32, device="cpu")]
        self.drop_path_hook = None          # tests: callable (layer, site, B) -> fp32 mask [B] (or None) in place of ops.bernoulli
        self.init_weights()

    # -- init -----------------------------------------------------------------------------------------------
    def init_weights(self):
        """maskclip_vit.py:378-429.  The pretrained CLIP file (pretrained/clip2mmseg_ViT16_clip_backbone.pth) is
        loaded (bicubic pos-embed resize included).  A configured-but-missing file raises, like mmcv's load_checkpoint:
        a silently random backbone -- and a random frozen clip_encoder feeding garbage MaskCLIP guidance -- is never
        what a training run wants.  `pretrained=None` (or allow_random_init=True) gives the reference's own random
        init (maskclip_vit.py:416-429)."""
        import os
        import warnings
        if isinstance(self.pretrained, str) and not os.path.exists(self.pretrained) and not self.allow_random_init:
            raise FileNotFoundError(
                f"pretrained weights '{self.pretrained}' not found (cwd {os.getcwd()}); convert them with "
                f"`python -m semivl_amd.tools.convert_clip_weights`, or pass allow_random_init=True "
                f"(cfg['allow_random_init']) for synthetic-weight benchmarking")
        if isinstance(self.pretrained, str) and os.path.exists(self.pretrained):
            ck = torch.load(self.pretrained, map_location="cpu")
            sd = ck.get("state_dict", ck)
            sd = {k.replace("backbone.", ""): v for k, v in sd.items()}
            if "pos_embed" in sd and sd["pos_embed"].shape != self.pos_embed.shape:
                n = int(math.sqrt(sd["pos_embed"].shape[1] - 1))
                h, w = self.img_size
                sd["pos_embed"] = self.resize_pos_embed(sd["pos_embed"], (h // self.patch_size, w // self.patch_size),
                                                        (n, n))
            if "proj.weight" in sd and sd["proj.weight"].dim() == 2:
                sd["proj.weight"] = sd["proj.weight"][:, :, None, None]
            res = self.load_state_dict(sd, strict=False)
            # (adapters keep LoRA.reset_parameters' init; the prompt tensors keep the constructor's: a CLIP file has neither)
            missing = [k for k in res.missing_keys if ".lora." not in k and
                       not k.startswith(("deep_prompt_embeddings", "prompt_proj.", "prompt_norm."))]
            if missing or res.unexpected_keys:
                warnings.warn(f"{self.pretrained}: missing keys {missing}, unexpected keys {res.unexpected_keys}")
            return
        with torch.no_grad():
            nn.init.trunc_normal_(self.pos_embed, std=.02)
            nn.init.trunc_normal_(self.cls_token, std=.02)
            for n, m in self.named_modules():
                if ".lora." in n:       # adapters keep LoRA.reset_parameters' init (b_* = 0: the model starts as its base)
                    continue
                if isinstance(m, nn.Linear):
                    nn.init.trunc_normal_(m.weight, std=.02)
                    if m.bias is not None:
                        if "ffn" in n:
                            nn.init.normal_(m.bias, mean=0., std=1e-6)
                        else:
                            nn.init.constant_(m.bias, 0)
                elif isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
                elif isinstance(m, nn.LayerNorm):
                    nn.init.constant_(m.weight, 1.0)
                    nn.init.constant_(m.bias, 0.)
                elif isinstance(m, _MHAParams):
                    nn.init.xavier_uniform_(m.in_proj_weight)
                    nn.init.constant_(m.in_proj_bias, 0.)

    @staticmethod
    def resize_pos_embed(pos_embed, hw, pos_hw):
        """maskclip_vit.py:460-490 (init-time / off-size inputs; host-side bicubic, not on the step's hot path)."""
        ph, pw = pos_hw
        cls_w = pos_embed[:, 0:1]
        w = pos_embed[:, -ph * pw:].reshape(1, ph, pw, pos_embed.shape[2]).permute(0, 3, 1, 2)
        w = F.interpolate(w, size=hw, mode="bicubic", align_corners=False)
        return torch.cat((cls_w, w.flatten(2).transpose(1, 2)), dim=1)

    # -- forward --------------------------------------------------------------------------------------------
    def _trainable(self):
        """Tensors the encoder's backward produces a gradient for.  prompt_norm.* is never among them: the reference's
        forward never calls it, so its .grad stays None there whatever requires_grad says."""
        never = set() if self.num_prompt_tokens is None else {id(t) for t in self.prompt_norm.parameters()}
        return [p for p in self.parameters() if p.requires_grad and id(p) not in never]

    def _check_grad_rules(self, params):
        """Every trainable tensor handed to the encoder's backward must have a gradient rule there: a tensor without one
        would silently never receive a gradient (AdamW skips it)."""
        ruled = self.__dict__.get("_ruled")
        if ruled is None:
            ruled = {id(t) for l_ in self.layers for t in l_.plist().values()}
            ruled |= {id(t) for l_ in self.layers if l_.lora is not None for t in l_.lora.parameters()}
            ruled |= {id(t) for t in (self.ln0.weight, self.ln0.bias, self.ln1.weight, self.ln1.bias, self.cls_token,
                                      self.pos_embed, self.patch_embed.projection.weight, self.proj.weight)}
            if self.num_prompt_tokens is not None:
                ruled |= {id(t) for t in (self.deep_prompt_embeddings, self.prompt_proj.weight, self.prompt_proj.bias)}
            self.__dict__["_ruled"] = ruled
        bad = [n for n, t in self.named_parameters() if t.requires_grad and id(t) not in ruled and
               any(t is q for q in params)]
        if bad:
            raise NotImplementedError(f"MaskClipVisionTransformer (HIP): no gradient rule for trainable {bad}")

    def _pos_resize_matrix(self, hw):
        """R [hw0*hw1, ph*pw] with resize_pos_embed(pos)[patches] == R @ pos[patches] (cached per target grid/device)."""
        Pz = self.patch_size
        ph, pw = self.img_size[0] // Pz, self.img_size[1] // Pz
        key = (hw, (ph, pw), str(self.pos_embed.device))
        cache = self.__dict__.setdefault("_pos_R", {})
        if key not in cache:
            with torch.no_grad():
                eye = torch.eye(ph * pw, device=self.pos_embed.device).view(ph * pw, 1, ph, pw)
                cache[key] = ops.StreamCached(
                    F.interpolate(eye, size=hw, mode="bicubic", align_corners=False).view(ph * pw, -1).t().contiguous())
        return cache[key].get()

    def forward_tokens(self, img, need_global=False, need_k=False):
        """Returns (feat_tokens list of [B, P, C] tensors, global or None) on the autograd graph.
        need_k: a third element, the LAST block's keys [B, P, E] without the class-token row (forward_qkv's k,
        maskclip_vit.py:110-118, 568-570), from the same encoder pass.  Gradient-free only."""
        tr = self._trainable()
        if need_k and self.num_prompt_tokens is not None:
            raise ValueError("MaskClipVisionTransformer.forward_tokens(need_k=True): num_prompt_tokens is set; the reference's "
                             "k[:, 1:] leaves the prompt rows among the keys, which no consumer here is defined on")
        Pz = self.patch_size
        hp, wp = (img.shape[2] + Pz - 1) // Pz, (img.shape[3] + Pz - 1) // Pz
        pos_in = None
        if hp * wp + 1 != self.pos_embed.shape[1]:
            # token count differs from the trained grid (e.g. 801 -> 816 -> 51x51 vs 50x50): per-forward bicubic resize
            # (maskclip_vit.py:447-459).  Bicubic interpolation is a fixed linear map of the patch positions: it is
            # tabulated once per (grid, grid') pair as a matrix R by pushing the identity through F.interpolate, and every
            # forward is then one GEMM R @ pos (backward R^T @ d) on the library -- ATen's bicubic kernel takes 6 ms on
            # this 7.7 MB tensor, 4 x per step.
            pos_in = _PosResizeFn.apply(self.pos_embed, self._pos_resize_matrix((hp, wp)))
            tr = [p for p in tr if p is not self.pos_embed]
        if torch.is_grad_enabled() and (tr or (pos_in is not None and pos_in.requires_grad)):
            if need_k:
                raise ValueError("MaskClipVisionTransformer.forward_tokens(need_k=True): autograd is enabled and the encoder "
                                 "has trainable tensors; the keys are gradient-free (call it under torch.no_grad())")
            outs = _EncoderFn.apply(self, img, need_global, pos_in, *tr)
        else:
            with ops.prof_scope("vit"):
                outs = _encoder_forward(self, img, need_global, None, pos_in, need_k=need_k)
        if need_k:
            return list(outs[:-2]), outs[-2], outs[-1]
        n = len(outs) - 1
        return list(outs[:n]), outs[n]

    def forward(self, inputs):
        """Reference-compatible output: [tuple(NCHW feats), global_embedding] (maskclip_vit.py:577-596).
        The NCHW tensors are zero-copy channels-last views of the token tensors."""
        feats, g = self.forward_tokens(inputs, need_global=True)
        B = inputs.shape[0]
        hp = (inputs.shape[2] + self.patch_size - 1) // self.patch_size
        wp = (inputs.shape[3] + self.patch_size - 1) // self.patch_size
        return [tuple(f.view(B, hp, wp, f.shape[-1]).permute(0, 3, 1, 2) for f in feats), g]


def _drop_path_masks(m, i, B, want_v, skip_x, dev):
    """Block i's live stochastic-depth sites for one forward: None (eval mode, or rate 0: the block runs as it does without the
    option), or dict(keep=, <site>=mask [B]).  One draw per sample and site, only for the branches this forward runs, in the
    reference's call order (v path first); drop_path_hook's mask takes precedence over the draw.  No device sync."""
    rate = m.dpr[i]
    if not (m.training and rate > 0):
        return None
    dp = dict(keep=1.0 - rate)
    for site in (("ffn_v",) if want_v else ()) + (() if skip_x else ("attn", "ffn")):
        mask = m.drop_path_hook(i, site, B) if m.drop_path_hook is not None else None
        if mask is None:
            mask = ops.bernoulli((B,), dp["keep"], dev)
        assert mask.dtype == torch.float32 and mask.numel() == B, (site, mask.shape, mask.dtype)
        dp[site] = mask.to(dev).contiguous().view(B)
    return dp


def _encoder_forward(m, img, need_global, saved, pos_in=None, need_k=False):
    assert img.is_cuda and img.dtype == torch.float32
    img = img.contiguous()
    B, Cin, H, W = img.shape
    Pz, E, L = m.patch_size, m.embed_dims, m.num_layers
    hp, wp = (H + Pz - 1) // Pz, (W + Pz - 1) // Pz  # 'corner' padding: bottom/right zero-fill up to a patch multiple
    NP = hp * wp
    T = NP + 1
    dev = img.device
    pos = m.pos_embed[0] if pos_in is None else pos_in.detach()
    assert pos.shape[0] == T, (pos.shape, T)
    x = ops.empty(B * T, E, device=dev)
    wpe = m.patch_embed.projection.weight.view(E, Cin * Pz * Pz)
    g = ops.conv_geom(H, W, Cin, Pz, Pz, patch=Pz)
    ops.gemm(ops.A_PATCH, ops.B_KC, B * NP, E, Cin * Pz * Pz, ops.Op(img, 0), ops.Op(wpe, Cin * Pz * Pz), x, ldc_m=E,
             out_mode=ops.OUT_PATCH, ct=(NP, 0, 0), conv=g, resid=pos, ldr_m=E)
    cls_row = ops.add(m.cls_token.view(E), pos[0])
    ops.copy2d(cls_row, 0, 1, 0, 0, x, 0, 1, T * E, 0, B, E)  # x[b*T] = cls + pos[0]
    x0, st0 = ops.layernorm_fwd(x, m.ln0.weight, m.ln0.bias, m.eps)
    # deep prompts: every block runs on TT = T + P rows per image, [class token | P prompt rows | patch tokens]; the patch
    # rows of a block's outputs start at row 1 + P
    P = m.num_prompt_tokens or 0
    TT = T + P
    if saved is not None:
        saved["x_pre"], saved["st0"] = x, st0
        if m.patch_embed.projection.weight.requires_grad:
            saved["img"] = img     # B operand of the patch-embedding weight gradient
        saved["layers"] = []
        saved["dims"] = (B, T, NP, hp, wp)      # (T without the prompt rows: the row count outside the blocks)
    x = x0
    if P:
        # prompt_proj over all layers' embeddings in one GEMM; one dropout mask per block and forward (independent per sample)
        pemb = ops.linear(m.deep_prompt_embeddings.detach().view(L * P, E), m.prompt_proj.weight, m.prompt_proj.bias)
        pmasks = [None] * L
        keep = 1.0 - m.prompt_dropout.p
        if m.training and not m.disable_dropout:
            for i in range(L):
                pmasks[i] = (m.prompt_mask_hook(i, B) if m.prompt_mask_hook is not None else ops.bernoulli((B, P, E), keep, dev))
        pscale = 1.0 / keep     # nn.Dropout's x * (mask / (1 - p)): the quotient is rounded to fp32 once, by the call
        if saved is not None:
            saved["prompt"] = (pmasks, pscale)
        x = ops.prompt_rows_fwd(pemb[:P], B, P, ops.empty(B * TT, E, device=dev), src=x0, mask=pmasks[0], scale=pscale)
    feats = []
    v_last = None
    for i, layer in enumerate(m.layers):
        last = i == L - 1
        want_v = m.return_qkv[i]
        skip_x = last and not need_global
        sv = {} if saved is not None else None
        pl = layer.plist() if layer.lora is None else layer.merged_plist()
        if P and i > 0:     # in place on the block above's output (no block keeps its own output for its backward)
            ops.prompt_rows_fwd(pemb[i * P:(i + 1) * P], B, P, x, mask=pmasks[i], scale=pscale)
        k_out = [] if need_k and last else None
        xo, v = block_forward(x, pl, m.num_heads, m.eps, B, TT, want_v, skip_x, sv, dp=_drop_path_masks(m, i, B, want_v, skip_x, dev),
                              k_out=k_out)
        if saved is not None:
            if layer.lora is not None:
                sv["plist"] = pl      # the backward's input-gradient GEMMs run on the same effective weights
            saved["layers"].append(sv)
        if i in m.out_indices:
            f = ops.empty(B * NP, E, device=dev)
            ops.copy2d(v, (1 + P) * E, NP, TT * E, E, f, 0, NP, NP * E, E, B * NP, E)  # v[:, 1 + P:]
            feats.append(f.view(B, NP, E))
        if last:
            v_last = v
        x = xo
    # tail: ln1 on v, proj 1x1, channel L2-normalise (maskclip_vit.py:537-555)
    vn, stv = ops.layernorm_fwd(v_last, m.ln1.weight, m.ln1.bias, m.eps)
    vtok = ops.empty(B * NP, E, device=dev)
    ops.copy2d(vn, (1 + P) * E, NP, TT * E, E, vtok, 0, NP, NP * E, E, B * NP, E)
    wproj = m.proj.weight.view(m.proj.weight.shape[0], E)
    pe = ops.linear(vtok, wproj)
    emb, inv = ops.l2norm_fwd(pe, 0.0)
    if saved is not None:
        saved.update(v_last=v_last, stv=stv, emb=emb, inv=inv)
        if m.proj.weight.requires_grad:
            saved["vtok"] = vtok   # B operand of the proj weight gradient
    if L in m.out_indices:
        feats.append(emb.view(B, NP, -1))
    glob = None
    if need_global:
        xn, _ = ops.layernorm_fwd(x, m.ln1.weight, m.ln1.bias, m.eps)
        c = ops.empty(B, E, device=dev)
        ops.copy2d(xn, 0, 1, TT * E, 0, c, 0, 1, E, 0, B, E)
        gp = ops.linear(c, wproj)
        glob, _ = ops.l2norm_fwd(gp, 0.0)
    if need_k:      # k[:, 1:] (maskclip_vit.py:570); P == 0 here (forward_tokens refuses prompts)
        return tuple(feats) + (glob, ops.group_rows(k_out[0], B, TT, 1, NP).view(B, NP, E))
    return tuple(feats) + (glob,)


def _sink_vectors(grads, pairs):
    """LayerNorm weight / bias gradients computed by layernorm_bwd(want_wgrad=True) into their sinks."""
    for prm, t in pairs:
        if prm.requires_grad:
            grads[id(prm)] = sink_grad(prm, lambda dst, acc, t=t: ops.add(dst, t, out=dst) if acc
                                       else ops.eltwise(4, t, None, out=dst))


class _PosResizeFn(torch.autograd.Function):
    """pos_embed [1, 1 + P, C] -> [1 + P', C] with the patch rows mapped through the tabulated bicubic matrix R [P', P]."""

    @staticmethod
    def forward(ctx, pos, R):
        ctx.R = R
        C = pos.shape[2]
        out = ops.empty(R.shape[0] + 1, C, device=pos.device)
        ops.eltwise(4, pos[0, 0].contiguous(), None, out=out[0])
        ops.matmul_nn(R, pos[0, 1:].contiguous(), out=out[1:])
        return out

    @staticmethod
    def backward(ctx, dout):
        R = ctx.R
        dout = dout.contiguous()
        C = dout.shape[1]
        dpos = ops.empty(1, R.shape[1] + 1, C, device=dout.device)
        ops.eltwise(4, dout[0].contiguous(), None, out=dpos[0, 0])
        ops.matmul_tn(R, dout[1:], out=dpos[0, 1:])
        return dpos, None


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, m, img, need_global, pos_in, *params):
        saved = {}
        with ops.prof_scope("vit"):
            outs = _encoder_forward(m, img, need_global, saved, pos_in)
        ctx.m, ctx.saved, ctx.need_global = m, saved, need_global
        ctx.pos_is_input = pos_in is not None
        ctx.n_feats = len(outs) - 1
        ctx.params = params
        m._check_grad_rules(params)
        gradsync.expect(params)
        if outs[-1] is not None:
            ctx.mark_non_differentiable(outs[-1])  # the global embedding is a side output (unused by VLGHead)
        return outs

    @staticmethod
    def backward(ctx, *douts):
        with ops.prof_scope("vit"):
            return _EncoderFn._backward(ctx, *douts)

    @staticmethod
    def _backward(ctx, *douts):
        m, s = ctx.m, ctx.saved
        B, T, NP, hp, wp = s["dims"]
        E, L = m.embed_dims, m.num_layers
        P = m.num_prompt_tokens or 0
        TT = T + P          # rows per image inside the blocks (prompt rows: 1 .. P)
        dev = s["x_pre"].device
        dfeats = list(douts[:ctx.n_feats])
        # map feature outputs back to (layer index) order
        feat_layers = [o for o in m.out_indices if o < L]
        has_emb = L in m.out_indices
        demb = dfeats[len(feat_layers)] if has_emb else None
        # ---- tail
        dv_last = None
        grads = {}
        if demb is not None:
            demb = demb.contiguous().view(B * NP, -1)
            dpe = ops.l2norm_bwd(demb, s["emb"], s["inv"])
            wproj = m.proj.weight.view(m.proj.weight.shape[0], E)
            dvtok = ops.matmul_nn(dpe, wproj)
            if m.proj.weight.requires_grad:
                vtok = s["vtok"]
                grads[id(m.proj.weight)] = sink_grad(m.proj.weight, lambda dst, acc: ops.matmul_tn(
                    dpe, vtok, out=dst.view(wproj.shape), accumulate=acc))
            dvn = ops.zeros(B * TT, E, device=dev)
            ops.copy2d(dvtok, 0, NP, NP * E, E, dvn, (1 + P) * E, NP, TT * E, E, B * NP, E)
            if m.ln1.weight.requires_grad or m.ln1.bias.requires_grad:
                dv_last, dg_, db_ = ops.layernorm_bwd(dvn, s["v_last"], s["stv"], m.ln1.weight, want_wgrad=True)
                _sink_vectors(grads, ((m.ln1.weight, dg_), (m.ln1.bias, db_)))
            else:
                dv_last = ops.layernorm_bwd(dvn, s["v_last"], s["stv"], m.ln1.weight)
        dvs = {L - 1: dv_last}
        for j, li in enumerate(feat_layers):
            d = dfeats[j]
            if d is None:
                continue
            d = d.contiguous().view(B * NP, E)
            full = ops.zeros(B * TT, E, device=dev)
            ops.copy2d(d, 0, NP, NP * E, E, full, (1 + P) * E, NP, TT * E, E, B * NP, E)
            dvs[li] = full if dvs.get(li) is None else ops.add(dvs[li], full)
        # ---- blocks, last to first
        dx = dxp = pend = None
        if P:
            # d emb_i = the batch sum of block i's input gradient on the prompt rows, of THIS backward call (the step runs
            # the encoder backward twice and main_grad accumulates: the three products below add each call's share once)
            pmasks, pscale = s["prompt"]
            ptrain = any(t.requires_grad for t in (m.deep_prompt_embeddings, m.prompt_proj.weight, m.prompt_proj.bias))
            pdemb = ops.zeros(L, P, E, device=dev) if ptrain else None
        for i in range(L - 1, -1, -1):
            layer = m.layers[i]
            sv = s["layers"][i]
            pl = layer.plist()
            want = frozenset(k_ for k_ in FFN_LN_KEYS if pl[k_].requires_grad)
            dx, dxp, g = block_backward(dx, dvs.get(i), sv.get("plist", pl), sv, m.num_heads, B, TT, want=want, dxo_p=dxp)
            if P and dx is not None:
                # the prompt rows of block i's input belong to emb_i alone: they are summed into pdemb[i] and do not flow
                # into block i - 1 (whose output prompt rows were discarded).  Block i - 1 packs its planes from the zeroed
                # fp32 matrix (dxp is dropped); block 0 hands the rows without the prompts to the ln0 backward.
                dxp = None
                d0 = ops.empty(B * T, E, device=dev) if i == 0 else None
                ops.prompt_rows_bwd(dx, B, P, out=pdemb[i] if ptrain else None, mask=pmasks[i], scale=pscale, compact=d0)
                if i == 0:
                    dx = d0
            # this block's weight gradients (two split-K GEMMs, their slab reductions, two column sums; with a trained FFN
            # two more GEMM families on B-operand producers) are off the dependency chain: they go to the weight-gradient
            # stream and run next to the chain's LayerNorm-backward / pack passes of the blocks below (ops.wgrad_side)
            used = [t_ for pair in g["wout_parts"] for t_ in pair] + [t_ for k_ in ("in_full", "in_v") for t_ in g.get(k_, ())]
            used += [t_ for k_ in want for part in g.get(k_, ()) for t_ in part[1:]]
            with ops.wgrad_side(*used):
                wg = attn_wgrads(layer, g, E)
                fg = ffn_ln_wgrads(pl, g) if want else {}
            a = layer.attn.attn
            grads[id(a.in_proj_weight)], grads[id(a.in_proj_bias)] = wg["win"], wg["bin"]
            grads[id(a.out_proj.weight)], grads[id(a.out_proj.bias)] = wg["wout"], wg["bout"]
            grads.update(wg.get("lora", ()))
            for k_, v_ in fg.items():
                grads[id(pl[k_])] = v_
            s["layers"][i] = None  # free this block's activations
            # this block's attention gradients are complete for this graph ONE BLOCK LATER (when its side-stream work has
            # had a block's time to finish): then their all-reduce bucket may go (train.py)
            if pend is not None:
                ops.wgrad_join(pend[0])
                gradsync.ready(pend[1])
            pend = (ops.wgrad_event(), [q for q in layer.parameters() if any(q is r_ for r_ in ctx.params)])
        ops.wgrad_join(produced=grads.values())     # every weight gradient of this graph is complete from here on
        if pend is not None:
            gradsync.ready(pend[1])
        if P and ptrain and dx is not None:
            df = pdemb.view(L * P, E)
            deep, w, bias = m.deep_prompt_embeddings, m.prompt_proj.weight, m.prompt_proj.bias
            if deep.requires_grad:      # emb = deep @ W^T + b
                grads[id(deep)] = sink_grad(deep, lambda dst, acc: ops.matmul_nn(df, w.detach(), out=dst.view(L * P, E), accumulate=acc))
            if w.requires_grad:
                dflat = deep.detach().view(L * P, E)
                grads[id(w)] = sink_grad(w, lambda dst, acc: ops.matmul_tn(df, dflat, out=dst, accumulate=acc))
            if bias.requires_grad:
                grads[id(bias)] = sink_grad(bias, lambda dst, acc: ops.colsum(df, out=dst, accumulate=acc))
        rest = [q for q in ctx.params if q is m.pos_embed or not any(q is r_ for l_ in m.layers for r_ in l_.parameters())]
        if dx is None:
            gradsync.ready(rest)
            ctx.saved = None
            return (None, None, None, None) + tuple(grads.get(id(p)) for p in ctx.params)
        # ---- ln0, pos_embed, cls_token, patch embedding
        if m.ln0.weight.requires_grad or m.ln0.bias.requires_grad:
            dxpre, dg_, db_ = ops.layernorm_bwd(dx, s["x_pre"], s["st0"], m.ln0.weight, want_wgrad=True)
            _sink_vectors(grads, ((m.ln0.weight, dg_), (m.ln0.bias, db_)))
        else:
            dxpre = ops.layernorm_bwd(dx, s["x_pre"], s["st0"], m.ln0.weight)
        if m.cls_token.requires_grad:   # x[b*T] = cls + pos[0]: the batch sum of the class-token rows
            grads[id(m.cls_token)] = sink_grad(m.cls_token, lambda dst, acc: ops.colsum(
                dxpre.view(B, T * E), out=dst.view(-1), accumulate=acc, C_=E, ld=T * E))
        wpe = m.patch_embed.projection.weight
        if wpe.requires_grad:           # patch tokens (rows b*T + 1 + p) against the image's patches
            dtok = ops.empty(B * NP, E, device=dev)
            ops.copy2d(dxpre, E, NP, T * E, E, dtok, 0, NP, NP * E, E, B * NP, E)
            img = s["img"]
            grads[id(wpe)] = sink_grad(wpe, lambda dst, acc: ops.matmul_tn_patch(
                dtok, img, m.patch_size, out=dst.view(E, -1), accumulate=acc))
        def pos_fn(dst, acc):
            # sum over the batch: rows b*T + t -> t
            ops.copy2d(dxpre, 0, B * T, 0, E, dst.view(-1), 0, T, 0, E, T, E, accumulate=acc)
            for b in range(1, B):
                ops.copy2d(dxpre, b * T * E, T, 0, E, dst.view(-1), 0, T, 0, E, T, E, accumulate=True)
        dpos_in = None
        if ctx.pos_is_input:  # resized pos_embed: hand the gradient back to torch autograd (bicubic backward)
            if m.pos_embed.requires_grad:
                dpos_in = ops.empty(T, E, device=dev)
                pos_fn(dpos_in, False)
        elif m.pos_embed.requires_grad:
            grads[id(m.pos_embed)] = sink_grad(m.pos_embed, pos_fn)
        gradsync.ready(rest)
        ctx.saved = None
        return (None, None, None, dpos_in) + tuple(grads.get(id(p)) for p in ctx.params)
