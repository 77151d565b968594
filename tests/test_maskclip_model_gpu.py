"""GPU: VLM + MaskClip2Head.  The tiny model against the reference's own float64 run (tests/golden/maskclip_refine.npz: VLM,
MaskClip2Head, forward_qkv and refine_output at the fixture's dimensions), one model at the real row geometry (E = 768, 12 heads,
32 x 32 tokens) against the float64 restatement applied to the model's own logits and keys under the kernels' bounds, the
backbone's key request, concept rows, train mode and the training steps' refusal.

Limits: cosine logits 1e-3 (the project's feature limit, max abs on unit-norm rows); a refined map 4 x the distance of the
reference's own float32 run from its float64 run (stored by the generator; never less than one fp32 rounding of 1), the rule
tests/test_text_kernels_gpu.py applies to QuickGELU; labels equal wherever the float64 top-2 gap exceeds twice that limit, the
excluded pixels at most 1 % (the generator asserts the reference's float32 run stays inside the same cap); keys 2e-3 relative to
the largest key, the limit tests/test_model_gpu.py holds linear-layer results to."""
import ast
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import maskclip_refine_ref as R
from golden_util import MCC_TEXT, TEXT, seeded_state

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
LOGIT_LIMIT = 1e-3
KEY_LIMIT = 2e-3
PAIRS = ((0.0, 0.0), (0.5, 0.0), (0.0, 0.7), (0.5, 0.7))


@pytest.fixture
def emu_mode():
    from semivl_amd import ops
    yield ops.set_gemm_emulation
    ops.set_gemm_emulation(0)


def build(S, embed, layers, heads, text=TEXT, nclass=21, clip=False, **head):
    from semivl_amd.model.builder import VLM, builtin_model_cfg
    m = copy.deepcopy(builtin_model_cfg("vlm-maskclip2-mcvitb"))["model"]
    m["backbone"].update(img_size=(S, S), embed_dims=embed, num_layers=layers, num_heads=heads, allow_random_init=True)
    m["decode_head"].update(img_size=S, num_classes=nclass, **head)
    m.pop("type")
    m.pop("pretrained")
    ccfg = None
    if clip:
        ccfg = copy.deepcopy(builtin_model_cfg("mcvit16"))["backbone"]
        ccfg.update(img_size=(S, S), embed_dims=embed, num_layers=layers, num_heads=heads, allow_random_init=True)
        ccfg.pop("pretrained")
    return VLM(load_text_embedding=text, load_mcc_text_embedding=text, load_pl_text_embedding=text, clip_encoder=ccfg, **m)


def spy(model):
    """Records what the head is handed and what it returns: dict x [B * HW, N], k [B * HW, E] or None, map [B, N, h, w]."""
    rec, head = {}, model.decode_head
    real = type(head).forward_tokens

    def forward_tokens(x, k, B, hw):
        out = real(head, x, k, B, hw)
        rec.update(x=x, k=k, map=out, hw=hw)
        return out

    head.forward_tokens = forward_tokens
    return rec


@pytest.fixture(scope="module")
def fix():
    z = np.load(os.path.join(HERE, "golden", "maskclip_refine.npz"), allow_pickle=False)
    return z, ast.literal_eval(str(z["model/cfg"]))


@pytest.fixture(scope="module")
def tiny(dev, fix):
    """The fixture's model and image, rebuilt from their seeds (checksums in the fixture)."""
    z, c = fix
    m = build(c["S"], c["embed"], c["layers"], c["heads"])
    assert len(m.decode_head.state_dict()) == 0 and all(k.startswith("backbone.") for k in m.state_dict())
    sd = seeded_state([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 500 + c["seed"])
    chk = np.array([sum(v.double().sum().item() for v in sd.values()), sum(v.double().abs().sum().item() for v in sd.values())])
    assert np.allclose(chk, z["model/w_checksum"], rtol=0, atol=1e-6), "seeded weight stream differs from the fixture's"
    m.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(100 + c["seed"])
    img = F.avg_pool2d(torch.randn(c["B"], 3, c["H"], c["W"], generator=g), 5, stride=1, padding=2)
    img = (img / img.std()).contiguous()
    assert np.allclose([img.double().sum().item(), img.double().abs().sum().item()], z["model/img_checksum"], rtol=0, atol=1e-6)
    return m.to(dev).eval(), img.to(dev)


@pytest.mark.parametrize("mode", [0, 6])
@pytest.mark.parametrize("pd,ks", PAIRS)
def test_tiny_model_against_the_reference(dev, fix, tiny, emu_mode, pd, ks, mode):
    z, c = fix
    m, img = tiny
    emu_mode(mode)
    head = m.decode_head
    head.pd_thresh, head.ks_thresh = pd, ks
    rec = spy(m)
    try:
        with torch.no_grad():
            out = m(img)
    finally:
        del head.forward_tokens
        head.pd_thresh = head.ks_thresh = 0.0
    tag = f"model/{pd}_{ks}"
    logits64 = torch.from_numpy(z["model/logits"])
    B, N, hp, wp = logits64.shape
    assert tuple(out.shape) == (B, N, c["H"], c["W"]) and rec["hw"] == (hp, wp)
    x = rec["x"].cpu().view(B, hp * wp, N).transpose(1, 2).reshape(B, N, hp, wp)
    e_logit = float((x.double() - logits64).abs().max())
    assert (rec["k"] is not None) == (ks > 0)
    want = torch.from_numpy(z[tag + "/map"])
    dist = float(z[tag + "/dist_f32"])
    limit = LOGIT_LIMIT if (pd, ks) == (0.0, 0.0) else 4.0 * max(dist, U)
    e_map = float((rec["map"].cpu().double() - want).abs().max())
    lab_limit = 4.0 * max(dist, U)
    gap = torch.from_numpy(z[tag + "/gap"]).double()
    excl = gap <= 2.0 * lab_limit
    labels = out.argmax(1).cpu()
    bad = (labels != torch.from_numpy(z[tag + "/labels"]).long()) & ~excl
    print(f"pd {pd} ks {ks} mode {mode}: logits {e_logit:.2e} (limit {LOGIT_LIMIT:.0e}, the reference's float32 run "
          f"{float(z['model/logits_dist_f32']):.2e}); map {e_map:.2e} (limit {limit:.2e}); excluded pixels {int(excl.sum())} of "
          f"{excl.numel()}, label mismatches outside {int(bad.sum())}")
    assert e_logit <= LOGIT_LIMIT
    if ks > 0:
        keys64 = torch.from_numpy(z["model/keys"])
        e_key = float((rec["k"].cpu().double().view_as(keys64) - keys64).abs().max() / keys64.abs().max())
        print(f"    keys {e_key:.2e} of the largest key (limit {KEY_LIMIT:.0e})")
        assert e_key <= KEY_LIMIT
    assert e_map <= limit
    assert float(excl.double().mean()) <= 0.01 and int(bad.sum()) == 0


def test_train_mode_returns_the_unrefined_logits_and_needs_no_keys(dev, tiny):
    m, img = tiny
    head = m.decode_head
    with torch.no_grad():
        plain = m(img)
    head.pd_thresh, head.ks_thresh = 0.5, 0.7
    rec = spy(m)
    try:
        m.train()
        assert not head.wants_keys()
        with torch.no_grad():
            got = m(img)
        assert rec["k"] is None and torch.equal(got, plain)
        out_g = m(img)                                    # grad mode on: still gradient-free, nothing trains
        assert not out_g.requires_grad and torch.equal(out_g, plain)
        m.eval()
        with torch.no_grad():
            refined = m(img)
        assert rec["k"] is not None and not torch.equal(refined, plain)
        for kw in (dict(need_fp=True), dict(only_fp=True)):
            with pytest.raises(NotImplementedError, match=next(iter(kw))):
                m(img, **kw)
    finally:
        del head.forward_tokens
        head.pd_thresh = head.ks_thresh = 0.0
        m.eval()


def test_both_training_steps_refuse_the_model(dev, tiny):
    from semivl_amd.train import semivl_train_step, supervised_train_step
    m, img = tiny
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for step in (semivl_train_step, supervised_train_step):
        with pytest.raises(ValueError, match="not trainable"):
            step(m, dict(img_x=img, mask_x=torch.zeros(img.shape[0], *img.shape[2:], dtype=torch.int64, device=dev)), 0, 10, {})
    assert not m.training and all(torch.equal(v, m.state_dict()[k]) for k, v in before.items())


def test_encoder_outputs_do_not_depend_on_the_key_request(dev, tiny):
    m, img = tiny
    with torch.no_grad():
        a = m.backbone.forward_tokens(img, need_global=True)
        b = m.backbone.forward_tokens(img, need_global=True, need_k=True)
        c_ = m.backbone.forward_tokens(img)
    assert len(a) == 2 and len(b) == 3 and len(c_) == 2 and c_[1] is None
    assert len(a[0]) == len(b[0]) == 1 and torch.equal(a[0][0], b[0][0]) and torch.equal(a[1], b[1]) and torch.equal(a[0][0], c_[0][0])
    hp, wp = (img.shape[2] + 15) // 16, (img.shape[3] + 15) // 16
    assert tuple(b[2].shape) == (img.shape[0], hp * wp, m.backbone.embed_dims)


@pytest.mark.parametrize("mode", [0, 6])
def test_block_keys_against_the_float64_restatement(dev, emu_mode, mode):
    """block_forward's k_out at the real width against F.linear in float64 (maskclip_refine_ref.keys_ref)."""
    from semivl_amd.model.vit import TransformerEncoderLayer, block_forward
    emu_mode(mode)
    g = torch.Generator().manual_seed(3)
    B, T, E, H = 2, 197, 768, 12
    layer = TransformerEncoderLayer(E, H, 4 * E, eps=1e-6)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.3) + (1.0 if n.endswith("ln1.weight") else 0.0))
    x = torch.randn(B, T, E, generator=g)
    a = layer.attn.attn
    with torch.no_grad():
        want = R.keys_ref(x.double(), layer.ln1.weight.double(), layer.ln1.bias.double(), 1e-6, a.in_proj_weight.double(),
                          a.in_proj_bias.double(), a.out_proj.weight.double(), a.out_proj.bias.double())
    layer.to(dev)
    k_out = []
    with torch.no_grad():
        _, v = block_forward(x.view(B * T, E).to(dev), layer.plist(), H, 1e-6, B, T, True, True, None, k_out=k_out)
        _, v0 = block_forward(x.view(B * T, E).to(dev), layer.plist(), H, 1e-6, B, T, True, True, None)
    assert len(k_out) == 1 and torch.equal(v, v0)
    got = k_out[0].cpu().view(B, T, E)[:, 1:].double()
    err = float((got - want).abs().max() / want.abs().max())
    print(f"block keys, mode {mode}: {err:.2e} of the largest key (limit {KEY_LIMIT:.0e})")
    assert err <= KEY_LIMIT


@pytest.mark.parametrize("mode", [0, 6])
def test_real_row_geometry_against_the_restatement(dev, emu_mode, mode):
    """E = 768, 12 heads, 2 layers, 32 x 32 tokens, B = 1, N = 21: the refined map against the float64 restatement applied to the
    model's OWN fp32 logits and keys, under the kernels' end-to-end bound.  The weights are random, so a row maximum may sit
    nearer to its threshold than P's bound: such rows (at most 1 %) are left out; a class peak that near fails the test.  At
    N = 21 the library serves both products from an fp32 kernel family in mode 6 too (tests/test_maskclip_refine_kernels_gpu.py
    prints the paths of this shape), so the fp32 bound holds in both modes; mode 6 changes the encoder that makes x and k."""
    torch.manual_seed(11)
    m = build(512, 768, 2, 12, pd_thresh=0.5, ks_thresh=0.7).to(dev).eval()
    emu_mode(mode)
    img = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(12)).to(dev)
    rec = spy(m)
    with torch.no_grad():
        out = m(img)
    B, HW, N, E = 1, 1024, 21, 768
    assert tuple(out.shape) == (1, N, 512, 512) and rec["hw"] == (32, 32)
    x, k = rec["x"].cpu().view(B, HW, N), rec["k"].cpu().view(B, HW, E)
    r = R.refine_ref(x, k, 0.5, 0.7)
    P64, pb = R.p_bound(x, r["dropped"])
    P0b = R.p_bound(x, torch.zeros_like(r["dropped"]))[1]
    assert bool(((r["peak"] - 0.5).abs() > P0b.view(B, HW, N).max(1).values).all()), "a class peak within P's bound of pd_thresh"
    safe = ((r["rowmax"] - 0.7).abs() > pb.view(B, HW, N).max(2).values).reshape(-1)
    assert float((~safe).double().mean()) <= 0.01
    s64 = R.s_ref(k.reshape(HW, E), B, HW)[0]
    W = r["W"]
    mag = k.double().abs() @ (s64.view(B, E, 1) * (k.double().abs().transpose(1, 2) @ P64.view(B, HW, N).abs()))
    bound = (R.SECOND * R.gamma(HW + E + 4) * mag + W.abs() @ pb.view(B, HW, N)).reshape(HW, N)
    sel = r["selected"].reshape(-1)
    bound = torch.where(sel[:, None], bound, pb)
    got = rec["map"].cpu().view(N, HW).t().double()
    want = r["out"][0].t()
    err = (got - want).abs()
    ratio = float((err[safe] / bound[safe].clamp_min(1e-300)).max())
    print(f"real row geometry, mode {mode}: dropped {int(r['dropped'].sum())} of {N}, smoothed {float(sel.double().mean()):.2f}, "
          f"unsafe rows {int((~safe).sum())}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_concept_rows_aggregate_to_forward_maskclips_classes(dev):
    """A text file with concept rows (98 rows for 21 classes): the head's map is the per-class maximum forward_maskclip takes."""
    from semivl_amd import ops
    from semivl_amd.model.text_embeddings import aggregate_concept_predictions, get_class_to_concept_idxs
    torch.manual_seed(5)
    m = build(64, 64, 2, 1, text=MCC_TEXT, clip=True)
    m.clip_encoder.load_state_dict(m.backbone.state_dict())
    m.to(dev).eval()
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(dev)
    rec = spy(m)
    with torch.no_grad():
        out = m(img)
        feats, _ = m.backbone.forward_tokens(img)
        emb = feats[-1]
        b, HW, Ce = emb.shape
        text = m._on("mcc", m.loaded_mcc_text_feat, dev)
        NC = text.shape[0]
        dense = ops.empty(b, NC, 4, 4, device=dev)
        ops.gemm(ops.A_KC, ops.B_KC, HW, NC, Ce, ops.Op(emb, Ce, 0, HW * Ce, 0), ops.Op(text, Ce), dense, ldc_m=1, ldc_n=HW,
                 batch=b, c_bso=NC * HW)                                       # forward_maskclip's own launch
        want = aggregate_concept_predictions(dense, get_class_to_concept_idxs(MCC_TEXT))
        labels = m.forward_maskclip(img, 0.0)
    assert NC == 98 and tuple(rec["x"].shape) == (b * HW, 21) and tuple(want.shape) == (b, 21, 4, 4)
    tol = 2 * R.gamma(Ce + 1)          # two fp32 products of unit vectors: each within gamma(K) of the exact cosine
    assert float((rec["map"] - want).abs().max()) <= tol
    t2 = out.topk(2, dim=1).values
    near = (t2[:, 0] - t2[:, 1]) <= 4 * tol
    assert bool((out.argmax(1) == labels)[~near].all()) and float(near.double().mean()) <= 0.05
