"""Golden-vector generator for the DeepLabV3+ ablation head (experiment 41, `vlm-dlv3p-bn12-sk4-{ft,ftap}-mcvitb`).
Runs ONLY where the reference tree exists, on the CPU: imports the reference's own `DLV3PHead` and `ASPPModule` (through
tests/golden/_ref_shim_dlv3p.py for the un-vendored mmseg base class), feeds them `forward_wrapper`'s need_fp concatenation
cat((f, dropout2d(f))) (builder.py:78-89) with fixed channel masks, and writes tests/golden/dlv3p_head.npz -- data only.

    python tests/golden/gen_golden_dlv3p.py

Per case (A: N = 5, 2 + 2 perturbed samples, map 24 x 20; B: N = 21, 1 + 1, map 32 x 32; the recipe's channel counts):
one train-mode forward + backward of the scalar loss sum(logits * G), then an eval-mode forward of the plain samples with
the running statistics that step left -- once in fp32 and once with the same modules in float64 (the noise floor).

Neither inputs nor parameters are stored (the 3x3 256 -> 256 weight alone is 2.4 MB): both are closed-form functions of the
flat element index (an integer hash, exact on every platform), written independently here and in tests/test_dlv3p_gpu.py.
Results with at most FULL_MAX elements are stored whole (fp32 run as float32, float64 run as float64).  Larger ones
(weight and input gradients, case B's logits) would not fit the size limit for committed files; of those the file holds
  sub / sub64   the values at SUB hashed positions (element-wise checks),
  sk  / sk64    a count sketch: SK buckets of signed sums, bucket and sign from the same hash.  For two tensors a, b
                E ||sk(a) - sk(b)||^2 = ||a - b||^2 with relative standard deviation sqrt(2 / SK) = 6 %: the relative L2
                distance of a whole tensor from the reference is measured from 4 KB,
  n2  / n2_64   the L2 norm of the whole tensor."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
M32 = 0xFFFFFFFF
FULL_MAX, SUB, SK = 10240, 1024, 512
CASES = dict(A=dict(N=5, n=2, H=24, W=20), B=dict(N=21, n=1, H=32, W=32))
C1, C4, C1P, DIL = 768, 512, 48, (6, 12, 18)


def hash32(i, salt):
    """i: uint64 array of flat indices -> uint64 array of 32-bit hashes (products wrap mod 2^64; the low 32 bits are exact)."""
    x = (i + np.uint64(salt) * np.uint64(0x9E3779B1)) & np.uint64(M32)
    x = (x * np.uint64(2654435761)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(M32)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(3266489917)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def salt_of(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name)) % 100003


def unit(n, name):
    """float64 [n] in [-1, 1): 2 * hash / 2^32 - 1."""
    return hash32(np.arange(n, dtype=np.uint64), salt_of(name)).astype(np.float64) / 2.0 ** 32 * 2.0 - 1.0


def param_value(name, shape):
    n = int(np.prod(shape))
    u = unit(n, name)
    if len(shape) == 4:                                  # conv weight: uniform, variance 2 / fan_in
        v = u * np.sqrt(6.0 / (shape[1] * shape[2] * shape[3]))
    elif name.endswith(".weight"):                       # BatchNorm scale
        v = 1.0 + 0.25 * u
    elif name.startswith("head.6"):                      # classifier bias
        v = 0.1 * u
    else:                                                # BatchNorm shift
        v = 0.25 * u
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def feature(name, n, HW, C):
    """Token layout [n, HW, C]: a per-element term plus a per-(sample, channel) offset (so the pooled branch is not ~ 0)."""
    v = unit(n * HW * C, name).reshape(n, HW, C) + unit(n * C, name + ".offset").reshape(n, 1, C)
    return torch.from_numpy(v.astype(np.float32))


def mask(name, n, C):
    return torch.from_numpy((unit(n * C, name) < 0.0).astype(np.float32).reshape(n, C))


def pack(out, key, t32, t64):
    a32, a64 = t32.detach().numpy().astype(np.float32).reshape(-1), t64.detach().numpy().astype(np.float64).reshape(-1)
    if a32.size <= FULL_MAX:
        out[key], out[key + "/f64"] = a32.reshape(t32.shape), a64.reshape(t64.shape)
        return
    i = np.arange(a32.size, dtype=np.uint64)
    pos = (hash32(np.arange(SUB, dtype=np.uint64), salt_of(key) + 1) % np.uint64(a32.size)).astype(np.int64)
    h = hash32(i, salt_of(key) + 2)
    bucket, sign = (h % np.uint64(SK)).astype(np.int64), 1.0 - 2.0 * ((h >> np.uint64(20)) & np.uint64(1)).astype(np.float64)
    for suf, a in (("", a32.astype(np.float64)), ("64", a64)):
        sk = np.zeros(SK)
        np.add.at(sk, bucket, sign * a)
        out[f"{key}/sk{suf}"] = sk
        out[f"{key}/n2{suf and '_64'}"] = np.float64(np.sqrt((a * a).sum()))
    out[key + "/sub"], out[key + "/sub64"] = a32[pos], a64[pos]
    out[key + "/shape"] = np.array(t32.shape, dtype=np.int64)


def run(head_cls, c, dtype):
    N, n, H, W = c["N"], c["n"], c["H"], c["W"]
    tag = f"{N}x{n}x{H}x{W}"
    head = head_cls(c1_in_channels=C1, c1_channels=C1P, dilations=DIL, img_size=16 * max(H, W), in_channels=C4,
                    in_index=3, channels=256, dropout_ratio=0, num_classes=N,
                    norm_cfg=dict(type="SyncBN", requires_grad=True), align_corners=False, init_cfg=None)
    with torch.no_grad():
        for name, p in head.named_parameters():
            p.copy_(param_value(name, tuple(p.shape)))
    head = head.to(dtype)
    keys = sorted(head.state_dict().keys())
    toks = dict(c1=feature(f"c1.{tag}", n, H * W, C1), c4=feature(f"c4.{tag}", n, H * W, C4))
    masks = dict(c1=mask(f"m1.{tag}", n, C1), c4=mask(f"m4.{tag}", n, C4))
    maps = {k: v.to(dtype).view(n, H, W, -1).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for k, v in toks.items()}
    # forward_wrapper, need_fp: cat((f, F.dropout2d(f, p = 0.5))) -- the mask injected, kept channels scaled by 1 / (1 - p)
    cat = {k: torch.cat((maps[k], maps[k] * masks[k].to(dtype)[:, :, None, None] * 2.0)) for k in maps}
    head.train()
    logits = head([cat["c1"], cat["c4"]])
    G = torch.from_numpy(unit(logits.numel(), f"G.{tag}").reshape(logits.shape)).to(dtype)
    (logits * G).sum().backward()
    res = {"logits_train": logits}
    for name, p in head.named_parameters():
        res["grad/" + name] = p.grad
    for k in maps:     # token layout, like the inputs
        res["grad_in/" + k] = maps[k].grad.permute(0, 2, 3, 1).reshape(n, H * W, -1)
    for name, b in head.named_buffers():
        res["stat/" + name] = b.detach().clone().to(torch.float64 if b.dtype.is_floating_point else b.dtype)
    head.eval()
    with torch.no_grad():
        res["logits_eval"] = head([maps["c1"].detach(), maps["c4"].detach()])
    return res, keys, masks


def main():
    os.chdir(REF)
    sys.path.insert(0, HERE)
    sys.path.insert(0, REF)
    import _ref_shim_dlv3p
    _ref_shim_dlv3p.install()
    from model.decode_heads.dlv3p_head import DLV3PHead
    from third_party.unimatch.model.semseg.deeplabv3plus import ASPPModule
    torch.manual_seed(0)
    out = {}
    for cname, c in CASES.items():
        r32, keys, masks = run(DLV3PHead, c, torch.float32)
        r64, _, _ = run(DLV3PHead, c, torch.float64)
        assert isinstance(DLV3PHead(c1_in_channels=8, c1_channels=4, dilations=DIL, img_size=32, in_channels=32, channels=8,
                                    num_classes=2).aspp, ASPPModule)
        out[f"{cname}/dims"] = np.array([c["N"], c["n"], c["H"], c["W"]], dtype=np.int64)
        for k, m_ in masks.items():
            out[f"{cname}/mask/{k}"] = m_.numpy().astype(np.uint8)
        for k in r32:
            if k.startswith("stat/") and not r32[k].dtype.is_floating_point:
                out[f"{cname}/{k}"] = r32[k].numpy()
            else:
                pack(out, f"{cname}/{k}", r32[k].float(), r64[k].double())
        worst = max(float((r32[k].double() - r64[k].double()).norm() / r64[k].double().norm()) for k in r32 if k.startswith("grad"))
        print(cname, "fp32 vs float64: logits max abs", float((r32["logits_train"].double() - r64["logits_train"]).abs().max()),
              "eval", float((r32["logits_eval"].double() - r64["logits_eval"]).abs().max()), "worst gradient rel-L2", worst)
    out["state_dict_keys"] = np.array(keys)
    path = os.path.join(HERE, "dlv3p_head.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
