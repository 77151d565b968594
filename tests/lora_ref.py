"""Float64 restatement of the two LoRA kernels (svl_lora_merge_f32, svl_lora_wgrad_f32) with the per-element sums of absolute
terms their rounding bounds are stated in, and the helpers the LoRA model tests share (the product model at the fixture's
dimensions with adapters, a per-case view of tests/golden/semivl_lora.npz)."""
import ast
import copy

import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative bound of n successive fp32 roundings"""
    return n * U / (1.0 - n * U)


def merge_ref(W, pairs, s):
    """W [n * rows, E], pairs[i] = (A [r, E], B [rows, r]) or None -> (Weff, mag) in float64:
    Weff = W + s * B @ A per row block (a block without a pair is W itself), mag = |W| + |s| * |B| @ |A|."""
    W = np.asarray(W, dtype=np.float64)
    n = len(pairs)
    rows = W.shape[0] // n
    out, mag = W.copy(), np.abs(W)
    for i, pr in enumerate(pairs):
        if pr is None:
            continue
        A, B = (np.asarray(t, dtype=np.float64) for t in pr)
        sl = slice(i * rows, (i + 1) * rows)
        out[sl] += s * (B @ A)
        mag[sl] += abs(s) * (np.abs(B) @ np.abs(A))
    return out, mag


def wgrad_ref(dW, A, B, s, dB0=None, dA0=None):
    """dW [rows, E], A [r, E], B [rows, r] -> (dB, dA, magB, magA) in float64: dB = dB0 + s * dW @ A^T,
    dA = dA0 + s * B^T @ dW (dB0 / dA0: what an accumulating call adds onto), mag*: the sums of absolute terms."""
    dW, A, B = (np.asarray(t, dtype=np.float64) for t in (dW, A, B))
    dB, dA = s * (dW @ A.T), s * (B.T @ dW)
    magB, magA = abs(s) * (np.abs(dW) @ np.abs(A).T), abs(s) * (np.abs(B).T @ np.abs(dW))
    if dB0 is not None:
        dB, magB = dB + np.asarray(dB0, dtype=np.float64), magB + np.abs(np.asarray(dB0, dtype=np.float64))
    if dA0 is not None:
        dA, magA = dA + np.asarray(dA0, dtype=np.float64), magA + np.abs(np.asarray(dA0, dtype=np.float64))
    return dB, dA, magB, magA


# ------------------------------------------------------------------------------------------------ model helpers
class Case:
    """The keys of one case ('A' / 'B') of semivl_lora.npz, with the shared ones (cfg, iters, fp_masks, in_checksum), behind
    the interface golden_util's fixture_* helpers read (z.files, z[key])."""

    def __init__(self, z, name):
        self.z, self.pre = z, name + "/"
        self.files = [k[len(self.pre):] for k in z.files if k.startswith(self.pre)] + [k for k in z.files if "/" not in k]
        self.spec = ast.literal_eval(str(z[self.pre + "case"]))

    def __getitem__(self, k):
        return self.z[self.pre + k] if (self.pre + k) in self.z.files else self.z[k]


def build_hip_lora(c, lora=None, **model_args):
    """The product model at the fixture's dimensions; `lora`: the lora_* kwargs merged into the backbone dict (what a model
    file under configs/_base_/models/ would carry), `model_args`: merged into the model dict (freeze_backbone, exclude_keys)."""
    from golden_util import MCC_TEXT, TEXT
    from semivl_amd.model.builder import VLM, builtin_model_cfg
    mcfg = copy.deepcopy(builtin_model_cfg("vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb"))["model"]
    ccfg = copy.deepcopy(builtin_model_cfg("mcvit16"))["backbone"]
    S = c["S"]
    for bb in (mcfg["backbone"], ccfg):
        bb.update(img_size=(S, S), embed_dims=c["embed"], num_layers=c["layers"], num_heads=c["heads"])
        bb.pop("pretrained", None)
    mcfg["backbone"]["out_indices"] = c["out_indices"]
    mcfg["backbone"].update(lora or {})
    mcfg["decode_head"].update(img_size=S, num_classes=21, text_channels=c["text_channels"], up_channels=c["up"],
                               skip_in_channels=(c["embed"], c["embed"]), skip_channels=c["skip"],
                               num_heads=c["dec_heads"], channels=c["channels"])
    mcfg.pop("type")
    mcfg.pop("pretrained", None)
    mcfg.update(model_args)
    return VLM(load_text_embedding=TEXT, load_mcc_text_embedding=MCC_TEXT, load_pl_text_embedding=TEXT,
               clip_encoder=ccfg, maskclip_class_filter=None, **mcfg)


def build_case(c, case):
    return build_hip_lora(c, case.spec["lora"], freeze_backbone=True, exclude_keys=case.spec["exclude_keys"])
