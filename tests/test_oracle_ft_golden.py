"""CPU: the oracle with every backbone tensor trainable (exclude_keys=("",), i.e. freeze_backbone=False) against the
fixture captured from the reference's own VLM built with freeze_backbone=False (tests/golden/gen_golden_ft.py)."""
import numpy as np
import torch

from golden_util import build_oracle, fixture_batch, fixture_fp_masks, fixture_state, load_fixture


def test_oracle_reproduces_reference_finetune_step(request):
    from oracle import semivl_oracle as O
    z, c = load_fixture("ft")
    request.addfinalizer(lambda n=torch.get_num_threads(): torch.set_num_threads(n))
    torch.set_num_threads(8)
    orc = build_oracle(c)
    orc.load_state_dict(fixture_state(z, c, orc), strict=True)
    for n, p in orc.backbone.named_parameters():       # VLM(exclude_keys=("",)): vlm.py:80-88 with a key every name holds
        p.requires_grad = any(k in n for k in ("",))
    batch = fixture_batch(z, c)
    masks = fixture_fp_masks(z, c)
    iters, total = [int(v) for v in z["iters"]]
    loss, aux = O.semivl_step(orc, batch, iters, total, conf_thresh=c["conf_thresh"], fp_masks=masks)
    loss.backward()
    assert abs(loss.item() - float(z["loss"])) < 1e-6
    for k in ("loss_x", "loss_s1", "loss_s2", "loss_fp", "loss_mc_s1", "loss_mc_s2", "loss_mc_fp"):
        assert abs(aux[k].item() - float(z[k])) < 1e-6, k
    grads = {k: p.grad for k, p in orc.named_parameters() if p.grad is not None}
    assert sorted(grads) == [str(s) for s in z["grad_names"]]
    # every backbone tensor reaches the loss in the reference: the whole ViT trains
    assert sorted(k for k in grads if k.startswith("backbone.")) == sorted("backbone." + n for n, _ in
                                                                          orc.backbone.named_parameters())
    for k, g in grads.items():
        ref = z["gnorm/" + k]
        assert abs(g.norm().item() - ref[0]) <= 1e-4 * max(ref[0], 1e-6) + 1e-9, k
    for f in z.files:
        if f.startswith("grad/"):
            k = f[5:]
            full = z[f]
            assert np.abs(grads[k].numpy() - full).max() <= 1e-4 * np.abs(full).max() + 1e-9, k
