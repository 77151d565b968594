"""Golden-vector generator for one SemiVL step with the OHEM supervised criterion (cfg['criterion'] = 'OHEM').  Runs ONLY
in the build container, like gen_golden.py: the 'tiny' fixture's reference model, weights, batch and dropout masks (the
same seeds, so semivl_tiny.npz's stored weights and inputs are this run's), the restated semivl.py:223-328 loop body
driven by the reference's own loss helpers, and criterion_l = the reference's own ProbOhemCrossEntropy2d
(third_party/unimatch/util/ohem.py) in place of nn.CrossEntropyLoss.  thresh sits in the widest gap of pred_x's
target-class probabilities (all near 1/21 at this initialisation: the gap is >= 4e-5, so every pixel is >= 2e-5 in p, a
logit change of ~4e-4, away from it) and min_kept below the count it keeps, so the selection is live: min_kept < kept <
valid.
Writes tests/golden/semivl_ohem.npz.

    python tests/golden/gen_golden_ohem_step.py
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
from golden_util import seeded_state  # noqa: E402

FULL = ("decode_head.head.weight", "decode_head.head.bias")


def main():
    os.chdir(G.REF)
    sys.path.insert(0, G.REF)
    import _ref_shim
    _ref_shim.install()
    from oracle import semivl_oracle as O
    import semivl as ref_semivl
    import utils.train_utils as ref_tu
    from third_party.unimatch.util.ohem import ProbOhemCrossEntropy2d

    def ref_cwl(loss, conf, ign, conf_mode, conf_thresh):
        return ref_tu.confidence_weighted_loss(loss, conf, ign, dict(conf_mode=conf_mode, conf_thresh=conf_thresh))

    def ref_mc(pred, mask, ign, reduce):
        ref_semivl.mcc_loss_reduce = reduce
        ref_semivl.criterion_mc = torch.nn.CrossEntropyLoss(ignore_index=255, reduction="none")
        return ref_semivl.compute_mc_loss(pred, mask, ign)

    helpers = (ref_tu.cutmix_img_, ref_tu.cutmix_mask, ref_cwl, ref_mc)
    c = G.CONFIGS["tiny"]
    torch.manual_seed(c["seed"])
    ref = G.build_reference(c)
    sd = seeded_state([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], c["seed"], c.get("logit_gain"))
    ref.load_state_dict(sd, strict=True)
    B, S = c["B"], c["S"]
    batch = O.synthetic_batch(B, S, 21, seed=1234 + c["seed"])
    g = torch.Generator().manual_seed(c["seed"] + 100)
    fp_masks = [(torch.rand(2 * B, ch, generator=g) > 0.5).float() for ch in (c["embed"], c["embed"], 512)]
    total_iters, iters = 100, 10

    class Adapter:
        def __init__(s, m):
            s.m = m

        def eval(s):
            s.m.eval()

        def train(s):
            s.m.train()

        def __call__(s, img, need_fp=False, fp_masks=None):
            return s.m(img, need_fp=need_fp)

        def forward_maskclip(s, img, t):
            return s.m.forward_maskclip(img, t)

    def run(criterion_l):
        """the loop body; the supervised term (the oracle's only cross entropy with ignore_index=255) goes through
        criterion_l when one is given"""
        ref.zero_grad()
        ref.load_state_dict(sd, strict=True)           # (BatchNorm running statistics: every run starts alike)
        feeder = G.MaskFeeder(fp_masks)
        orig_do, orig_F = F.dropout2d, O.F
        F.dropout2d = feeder
        if criterion_l is not None:
            O.F = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("__")})
            O.F.cross_entropy = lambda p, t, **kw: (criterion_l(p, t) if kw == {"ignore_index": 255} else
                                                    F.cross_entropy(p, t, **kw))
        try:
            loss, aux = O.semivl_step(Adapter(ref), batch, iters, total_iters, conf_thresh=c["conf_thresh"],
                                      fp_masks=fp_masks, helpers=helpers)
        finally:
            F.dropout2d, O.F = orig_do, orig_F
        loss.backward()
        return loss.detach(), aux, {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}

    # pick thresh / min_kept on pred_x of a plain run (the OHEM relabelling does not change the forward)
    _, aux0, _ = run(None)
    px, mx = aux0["pred_x"].detach(), batch["mask_x"]
    valid = mx != 255
    p = F.softmax(px, dim=1).gather(1, (mx * valid).unsqueeze(1)).squeeze(1)[valid].double().sort().values
    print("p quantiles", [round(float(p[int(q * (len(p) - 1))]), 6) for q in (0, 0.01, 0.1, 0.5, 0.9, 0.99, 1)])
    lo, hi = p[int(0.05 * len(p))], p[int(0.995 * len(p))]
    gaps, mid = p[1:] - p[:-1], 0.5 * (p[1:] + p[:-1])
    gaps = torch.where((mid > lo) & (mid < hi), gaps, torch.zeros_like(gaps))
    j = int(gaps.argmax())
    assert gaps[j] >= 4e-5, float(gaps[j])
    thresh = round(float(mid[j]), 6)
    min_kept = int((p <= thresh).sum()) // 2
    print(f"thresh {thresh} (gap {float(gaps[j]):.2e}), min_kept {min_kept}, valid {len(p)}")

    crit = ProbOhemCrossEntropy2d(255, thresh=thresh, min_kept=min_kept)
    seen = {}
    crit.criterion.register_forward_pre_hook(lambda m_, args: seen.update(t=args[1].clone()))
    rl, raux, rg = run(crit)
    kept = int((seen["t"] != 255).sum())
    assert min_kept < kept < len(p), (min_kept, kept, len(p))
    print(f"loss {rl.item():.8f} loss_x {raux['loss_x'].item():.8f} kept {kept}")
    out = dict(criterion=np.array(repr(dict(name="OHEM", kwargs=dict(ignore_index=255, thresh=thresh, min_kept=min_kept)))),
               iters=np.array([iters, total_iters]), loss=rl.numpy(),
               **{k: raux[k].detach().numpy() for k in ("loss_x", "loss_s1", "loss_s2", "loss_fp", "loss_mc_s1",
                                                         "loss_mc_s2", "loss_mc_fp")},
               mask_x_ohem=seen["t"].numpy().astype(np.uint8), grad_names=np.array(sorted(rg)))
    for k in sorted(rg):
        out["gnorm/" + k] = np.array([rg[k].norm().item(), rg[k].flatten()[0].item(), rg[k].flatten()[-1].item()])
    for k in FULL:
        out["grad/" + k] = rg[k].numpy()
    path = os.path.join(HERE, "semivl_ohem.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
