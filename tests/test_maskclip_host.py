"""CPU: the zero-shot MaskCLIP model part builds -- by its built-in name and from a model file in the working directory --,
MaskClip2Head validates its thresholds and holds no tensors, the backbone refuses the key request where it must, the training
steps refuse the head before touching anything, and the model names the project pins as unsupported keep raising."""
import os

import pytest
import torch

CFG = dict(model="mmseg.vlm-maskclip2-mcvitb", nclass=21, crop_size=512, dataset="pascal", text_embedding_variant="single",
           mcc_text="concept4_single", pl_text="single", disable_dropout=True, fp_rate=0.5, allow_random_init=True)

MODEL_FILE = '''
img_size = 64
model = dict(type="VLM", backbone=dict(type="MaskClipVisionTransformer", img_size=(64, 64), patch_size=16, patch_bias=False,
                                       in_channels=3, embed_dims=64, num_layers=2, num_heads=1, mlp_ratio=4, out_indices=None,
                                       qkv_bias=True, with_cls_token=True, norm_cfg=dict(type="LN", eps=1e-6),
                                       act_cfg=dict(type="GELU"), pre_norm=True, final_norm=True, return_clip_embed=True,
                                       return_qkv=True, interpolate_mode="bicubic"),
             decode_head=dict(type="MaskClip2Head", img_size=64, in_channels=512, channels=512, num_classes=19,
                              align_corners=False, in_index=-1, pd_thresh=0.5, ks_thresh=0.7, dropout_ratio=0,
                              loss_decode=dict(type="CrossEntropyLoss"), norm_cfg=dict(type="SyncBN")),
             freeze_backbone=True)
'''


def test_builtin_name_builds():
    from semivl_amd.model.builder import build_model, builtin_model_cfg
    from semivl_amd.model.maskclip_head import MaskClip2Head
    m = build_model(dict(CFG))
    assert isinstance(m.decode_head, MaskClip2Head)
    assert (m.num_classes, m.decode_head.image_size, m.align_corners) == (21, 512, False)
    assert (m.decode_head.pd_thresh, m.decode_head.ks_thresh) == (0.0, 0.0)
    assert m.backbone.out_indices == [12] and m.clip_encoder is None
    assert m.head_res_size((512, 512)) is None
    assert not any(p.requires_grad for p in m.parameters())
    c = builtin_model_cfg("vlm-maskclip2-mcvitb")["model"]
    assert c["pretrained"] == "pretrained/clip2mmseg_ViT16_clip_backbone.pth" and c["decode_head"]["in_index"] == -1
    with pytest.raises(FileNotFoundError):           # without allow_random_init the CLIP file is required
        build_model({k: v for k, v in CFG.items() if k != "allow_random_init"})


def test_model_file_in_the_working_directory(tmp_path, monkeypatch):
    from semivl_amd.model.builder import build_model
    d = tmp_path / "configs" / "_base_" / "models"
    d.mkdir(parents=True)
    (d / "vlm-maskclip2-tiny.py").write_text(MODEL_FILE)
    monkeypatch.chdir(tmp_path)
    m = build_model(dict(CFG, model="mmseg.vlm-maskclip2-tiny", crop_size=64))
    h = m.decode_head
    assert (h.pd_thresh, h.ks_thresh, h.num_classes, h.image_size) == (0.5, 0.7, 21, 64)
    assert h.wants_keys() is False                   # a fresh module is in train mode: no refinement, no keys
    m.eval()
    assert h.wants_keys() is True
    m2 = build_model(dict(CFG, model="mmseg.vlm-maskclip2-tiny", crop_size=64,
                          model_args={"decode_head": dict(type="MaskClip2Head", img_size=64, in_channels=512, channels=512,
                                                          num_classes=21, ks_thresh=0.0)}))
    assert m2.eval().decode_head.wants_keys() is False


def test_head_has_no_tensors_and_validates_thresholds():
    from semivl_amd.model.builder import build_head
    from semivl_amd.model.maskclip_head import MaskClip2Head
    h = build_head(dict(type="MaskClip2Head", img_size=32, in_channels=512, channels=512, num_classes=5))
    assert isinstance(h, MaskClip2Head) and len(h.state_dict()) == 0 and not list(h.parameters()) and not list(h.buffers())
    assert MaskClip2Head(32, 512, 512, 5, pd_thresh=1, ks_thresh=0.25).pd_thresh == 1.0
    for bad in (-0.1, True, False, "0.5", None, float("nan"), [0.5]):
        for key in ("pd_thresh", "ks_thresh"):
            with pytest.raises(ValueError, match=key):
                MaskClip2Head(32, 512, 512, 5, **{key: bad})
    with pytest.raises(RuntimeError, match="not trainable"):
        h.forward_train(None, None, None, None)


def test_key_request_refusals_name_their_reason():
    from semivl_amd.model.vit import MaskClipVisionTransformer
    kw = dict(img_size=32, patch_size=16, patch_bias=False, embed_dims=64, num_layers=2, num_heads=1, out_indices=None,
              pre_norm=True, final_norm=True, return_clip_embed=True, return_qkv=True, norm_cfg=dict(type="LN", eps=1e-6),
              allow_random_init=True)
    img = torch.zeros(1, 3, 32, 32)
    with pytest.raises(ValueError, match="num_prompt_tokens"):
        MaskClipVisionTransformer(num_prompt_tokens=2, **kw).forward_tokens(img, need_k=True)
    vit = MaskClipVisionTransformer(**kw)
    assert any(p.requires_grad for p in vit.parameters())
    with pytest.raises(ValueError, match="autograd is enabled"):
        vit.forward_tokens(img, need_k=True)


@pytest.mark.parametrize("step", ["semivl_train_step", "supervised_train_step"])
def test_training_steps_refuse_the_head_before_touching_anything(step):
    import semivl_amd.train as T
    from semivl_amd.model.maskclip_head import MaskClip2Head

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.decode_head = MaskClip2Head(32, 512, 512, 5)

    class Untouchable(dict):
        def __getitem__(self, k):
            raise AssertionError("the step read the batch")

    with pytest.raises(ValueError, match="not trainable"):
        getattr(T, step)(Holder(), Untouchable(), 0, 10, Untouchable())


@pytest.mark.parametrize("model", ["mmseg.vlm-dlv3p-bn11-sk4-ft-tvit-in1k", "mmseg.vlm-zegclip-rd-pt-vitb", "deeplabv3plus"])
def test_pinned_unsupported_names_still_raise(model):
    from semivl_amd.model.builder import build_model
    with pytest.raises(ValueError):
        build_model(dict(CFG, model=model))


def test_unknown_head_type_is_still_a_key_error():
    from semivl_amd.model.builder import build_head
    with pytest.raises(KeyError):
        build_head(dict(type="MaskClipHead", img_size=32))
