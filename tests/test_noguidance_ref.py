"""CPU: the restated loops of tests/noguidance_ref.py (semivl.py:223-328 along its `lambda == 0` branches, supervised.py:
277-289), driven in float64 with the oracle's modules, against tests/golden/semivl_noguidance.npz -- the float64 run of the
reference's own modules (tests/golden/gen_golden_noguidance.py).  Limit 1e-12, relative to max(1, |reference|) for scalars
and to the tensor's largest magnitude for gradients; label maps bit-exact.  Weights and inputs are regenerated from the seeds
and their checksums compared with the fixture's."""
import ast
import contextlib
import os

import numpy as np
import torch

import noguidance_ref as R
from golden_util import HERE, MCC_TEXT, fixture_batch, fixture_fp_masks, fixture_state, text_feats

TOL = 1e-12


def load():
    z = np.load(os.path.join(HERE, "golden", "semivl_noguidance.npz"), allow_pickle=False)
    return z, ast.literal_eval(str(z["cfg"]))


def build_oracle_unguided(c):
    from oracle import semivl_oracle as O
    from semivl_amd.model.text_embeddings import get_class_to_concept_idxs
    t, m = text_feats()
    orc = O.build_vlm(dict(nclass=21, crop=c["S"], embed=c["embed"], layers=c["layers"], heads=c["heads"],
                           out_indices=tuple(c["out_indices"]), channels=c["channels"], text_channels=c["text_channels"],
                           up=c["up"], skip_in=(c["embed"], c["embed"]), skip=c["skip"]), t, m,
                      get_class_to_concept_idxs(MCC_TEXT))
    for lyr in orc.decode_head.layers:
        lyr.transformer.attn.attn.num_heads = c["dec_heads"]
    orc.clip_encoder = None         # experiments.py:197-202
    return orc


@contextlib.contextmanager
def float64():
    """Default dtype float64 and `.float()` keeping float64 (the oracle casts the fp16 text embedding with it), as in the
    generator's float64 run.  Entered AFTER weights and inputs are seeded: their streams are float32 draws."""
    keep = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.Tensor.float = keep
        torch.set_default_dtype(torch.float32)


def _model_and_batch(z, c):
    orc = build_oracle_unguided(c)
    sd = fixture_state(z, c, orc)             # (asserts the weight checksum)
    assert list(sd) == [str(k) for k in z["state_keys"]] and not any(k.startswith("clip_encoder.") for k in sd)
    orc.load_state_dict(sd, strict=True)
    orc.double()
    assert all(p.dtype == torch.float64 for p in orc.parameters())
    batch = fixture_batch(z, c)               # (asserts the input checksum)
    return orc, {k: v.double() if v.is_floating_point() else v for k, v in batch.items()}


def _check_grads(z, pre, grads):
    assert sorted(grads) == [str(s) for s in z[pre + "grad_names"]]
    for k, g in grads.items():
        ref = z[pre + "gnorm/" + k]
        assert abs(g.norm().item() - ref[0]) <= TOL * max(ref[0], 1.0), (k, g.norm().item(), ref[0])
    for k in R.GRAD_FULL:
        full = z[pre + "grad/" + k]
        assert np.abs(grads[k].numpy() - full).max() <= TOL * max(np.abs(full).max(), 1.0), k


def test_case_a_semisupervised_step():
    z, c = load()
    orc, batch = _model_and_batch(z, c)
    masks = [m.double() for m in fixture_fp_masks(z, c)]
    with float64():
        loss, aux = R.semivl_step_unguided(orc, batch, c["conf_thresh"], "pixelwise", masks)
        loss.backward()
    assert loss.dtype == torch.float64
    for k, v in (("loss", loss), *((k, aux[k]) for k in ("loss_x", "loss_s1", "loss_s2", "loss_fp"))):
        assert abs(v.item() - float(z["A/" + k])) <= TOL * max(1.0, abs(float(z["A/" + k]))), (k, v.item(), float(z["A/" + k]))
    for k in ("mask_w", "mask_w_other"):
        assert np.array_equal(aux[k].numpy().astype(np.uint8), z["A/" + k]), k
    _check_grads(z, "A/", R.grads_of(orc))


def test_case_c_supervised_step():
    z, c = load()
    orc, batch = _model_and_batch(z, c)
    with float64():
        loss, pred = R.supervised_step(orc, batch)
        loss.backward()
    assert abs(loss.item() - float(z["C/loss"])) <= TOL * max(1.0, abs(float(z["C/loss"])))
    ref = z["C/pred_x_s16"]
    assert np.abs(pred.detach()[:, :, ::16, ::16].numpy() - ref).max() <= TOL * np.abs(ref).max()
    _check_grads(z, "C/", R.grads_of(orc))
    # the supervised loss is the semi-supervised step's loss_x: same model, same labelled half
    assert abs(float(z["C/loss"]) - float(z["A/loss_x"])) <= TOL * abs(float(z["C/loss"]))
