"""SHA-256 digests of what the fused optimizers compute on the tiny fixture model, to compare two commits bit for bit (no
training step runs).  Three constructions with ema_decay 0.99 -- FusedAdamW(exp 40), build_optimizer(SGD, nesterov, exp 40's
custom keys), FusedSGD.original -- each through four rounds of: seeded gradients into the arena, a `.grad` on one arena
parameter (so the fold runs), step(), poly_lr(); after two rounds the state moves through state_dict() into a fresh optimizer.
usage: python tools/optim_digest.py [--out FILE.json]"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from golden_util import build_hip, fixture_state, load_fixture  # noqa: E402
from semivl_amd.synthetic import exp40_cfg  # noqa: E402
from semivl_amd.train import FusedAdamW, FusedSGD, build_optimizer  # noqa: E402

OCFG = exp40_cfg()["optimizer"]
CK = OCFG["paramwise_cfg"]["custom_keys"]
BUILD = {
    "FusedAdamW": lambda model: FusedAdamW(model, OCFG, ema_decay=0.99),
    "FusedSGD": lambda model: build_optimizer(model, dict(type="SGD", lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4,
                                                          paramwise_cfg=dict(custom_keys=CK)), ema_decay=0.99),
    "FusedSGD.original": lambda model: FusedSGD.original(model, 0.001, 10.0, ema_decay=0.99),
}


def sha(t):
    t = t.detach().cpu().reshape(-1)
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def plain(x):
    """Tensors -> (dtype, shape, digest), dicts -> sorted item lists: something repr() writes the same way every time."""
    if torch.is_tensor(x):
        return (str(x.dtype), tuple(x.shape), sha(x))
    if isinstance(x, dict):
        return sorted(((repr(k), plain(v)) for k, v in x.items()))
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return repr(x)


def fresh(build, dev):
    z, c = load_fixture("tiny")
    model = build_hip(c)
    model.load_state_dict(fixture_state(z, c, model), strict=True)
    return build(model.to(dev))


def run(build, dev):
    opt = fresh(build, dev)
    for k in range(4):
        if k == 2:      # the hand-over of a resumed run: parameters and teacher from the checkpoint, the rest from the dict
            old, opt = opt, fresh(build, dev)
            opt.p.copy_(old.p)
            opt.ema.copy_(old.ema)
            opt.load_state_dict(old.state_dict())
        torch.manual_seed(k)
        opt.g.copy_(torch.randn(opt.total) * 0.1)
        prm = opt.groups[1]["param"]
        prm.grad = (torch.randn(prm.shape) * 0.1).to(dev)
        opt.step()
        opt.poly_lr(k, 50, warmup_iters=2)
    torch.cuda.synchronize()
    bufs = dict(p=opt.p, g=opt.g, m=getattr(opt, "m", None), v=getattr(opt, "v", None), ema=opt.ema, seg_lr=opt.seg_lr)
    out = {k: sha(t) for k, t in bufs.items() if t is not None}
    out["state_dict"] = hashlib.sha256(repr(plain(opt.state_dict())).encode()).hexdigest()
    out["step_count"], out["total"] = opt.step_count, opt.total
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), digests={name: run(build, dev) for name, build in BUILD.items()})
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
