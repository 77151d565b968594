"""Golden-vector generator for the OHEM supervised criterion (cfg['criterion'] = 'OHEM', semivl.py:142-149,267).  Runs ONLY
in the build container, like gen_golden.py: it imports the reference's own ProbOhemCrossEntropy2d
(third_party/unimatch/util/ohem.py), applies it to F.interpolate(low-resolution logits) as the loop applies it to pred_x,
and writes tests/golden/ohem_cases.npz with, per case, the inputs, the loss, the relabelled target (the argument handed
to the criterion's inner nn.CrossEntropyLoss) and d(loss)/d(low-resolution logits).

Away from the deliberate-tie case every threshold that decides (thresh, or the k-th smallest probability) sits in a gap of
the probabilities >= 2e-5 wide, so ulp-level differences between implementations cannot move a pixel across it.

    python tests/golden/gen_golden_ohem.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
GAP = 2e-5


def target_prob(full, target):
    """ohem.py:36-45 in float32: softmax at the target class, 1.0 at ignored pixels."""
    valid = target != 255
    p = F.softmax(full, dim=1).gather(1, (target * valid).unsqueeze(1)).squeeze(1)
    return torch.where(valid, p, torch.ones_like(p))


def gap_around(vals, x):
    """distance from x to the nearest probability value other than x itself"""
    d = (vals - x).abs()
    d = d[d > 0]
    return float(d.min()) if d.numel() else 1.0


def thresh_in_gap(vals, lo_q, hi_q):
    """the middle of the widest gap between consecutive sorted values inside the [lo_q, hi_q] quantile range"""
    s = vals.double().sort().values
    lo, hi = s[int(lo_q * (len(s) - 1))], s[int(hi_q * (len(s) - 1))]
    gaps = s[1:] - s[:-1]
    mid = 0.5 * (s[1:] + s[:-1])
    gaps = torch.where((mid > lo) & (mid < hi), gaps, torch.zeros_like(gaps))
    j = int(gaps.argmax())
    t = round(float(mid[j]), 7)
    assert gaps[j] >= 2 * GAP and gap_around(s, t) >= GAP, (float(gaps[j]), t)
    return t


def main():
    sys.path.insert(0, REF)
    from third_party.unimatch.util.ohem import ProbOhemCrossEntropy2d

    cases = [
        # name, N, B, h, w, scale, align, ignore fraction, kind
        ("kth_binds", 5, 2, 8, 8, 4, False, 0.1, "kth"),
        ("thresh_binds", 21, 2, 6, 8, 4, False, 0.1, "thresh"),
        ("min_kept_gt_valid", 5, 2, 8, 8, 2, True, 0.3, "gt_valid"),
        ("min_kept_zero", 21, 1, 8, 8, 4, False, 0.1, "zero"),
        ("min_kept_gt_numel", 21, 2, 8, 6, 2, False, 0.0, "gt_numel"),
        ("ties", 5, 2, 8, 8, 4, False, 0.05, "ties"),
        ("heavy_ignore", 21, 2, 8, 8, 4, True, 0.6, "kth"),
    ]
    out = {}
    g = torch.Generator().manual_seed(2024)
    for i, (name, N, B, h, w, r, align, ign_frac, kind) in enumerate(cases):
        H, W = h * r, w * r
        low = (torch.randn(B, N, h, w, generator=g) * 3.0).float()
        if kind == "ties":
            low[:, :, : h // 2] = 0.0        # uniform logits: every pixel whose taps all lie there has p = 1 / N exactly
        target = torch.randint(0, N, (B, H, W), generator=g)
        target[torch.rand(B, H, W, generator=g) < ign_frac] = 255
        full = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=align)
        with torch.no_grad():
            p = target_prob(full, target).flatten()
        n, nv = p.numel(), int((target != 255).sum())
        s = p.double().sort().values
        if kind == "kth":          # v = s[k - 1] > thresh, and s[k] (the next larger value) is >= GAP above v
            thresh = thresh_in_gap(p, 0.02, 0.15)
            cand = [k for k in range(int(0.3 * n), int(0.6 * n)) if s[k] - s[k - 1] >= GAP and s[k - 1] - s[k - 2] >= GAP]
            min_kept = cand[len(cand) // 2]
            assert s[min_kept - 1] > thresh
        elif kind == "thresh":     # the k-th value lies below thresh
            thresh = thresh_in_gap(p, 0.4, 0.6)
            min_kept = int(0.1 * n)
            assert s[min_kept - 1] < thresh
        elif kind == "gt_valid":
            thresh, min_kept = 0.7, nv + 5
        elif kind == "zero":
            thresh, min_kept = thresh_in_gap(p, 0.4, 0.6), 0
        elif kind == "gt_numel":
            thresh, min_kept = thresh_in_gap(p, 0.4, 0.6), n + 100
        else:                      # ties: the k-th value is the tied 1 / N; thresh lies below it
            tie = float(F.softmax(torch.zeros(1, N), dim=1)[0, 0])
            lt, le = int((p < tie).sum()), int((p <= tie).sum())
            assert le - lt > 100, (lt, le)
            assert gap_around(s, tie) >= GAP
            min_kept = (lt + le) // 2
            thresh = thresh_in_gap(p[p < tie], 0.3, 0.7)
        low_r = low.clone().requires_grad_(True)
        crit = ProbOhemCrossEntropy2d(255, thresh=thresh, min_kept=min_kept)
        seen = {}
        crit.criterion.register_forward_pre_hook(lambda m_, args: seen.update(t=args[1].clone()))
        loss = crit(F.interpolate(low_r, size=(H, W), mode="bilinear", align_corners=align), target)
        loss.backward()
        kept = int((seen["t"] != 255).sum())
        print(f"[{name}] N={N} B={B} {h}x{w}->{H}x{W} align={align} n={n} valid={nv} thresh={thresh} "
              f"min_kept={min_kept} kept={kept} loss={loss.item():.6f}")
        pre = f"c{i}/"
        out.update({pre + "name": np.array(name), pre + "logits": low.numpy(), pre + "target": target.numpy().astype(np.uint8),
                    pre + "geom": np.array([H, W, int(align)]), pre + "thresh": np.array(thresh),
                    pre + "min_kept": np.array(min_kept), pre + "loss": np.array(loss.item()),
                    pre + "relabel": seen["t"].numpy().astype(np.uint8), pre + "grad": low_r.grad.numpy()})
    out["num_cases"] = np.array(len(cases))
    path = os.path.join(HERE, "ohem_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
