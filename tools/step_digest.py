"""What the two training steps compute AND launch on the tiny fixture model, to compare two versions of semivl_amd/train.py:
per case (two consecutive steps, FusedAdamW with an EMA arena, return_aux=True) the SHA-256 of the loss tensor, of every aux
tensor and of the optimizer's p / g / ema arenas after the second step, and the ordered list of library calls (every call goes
through semivl_amd.lib.check, whose `what` is the call's name) tagged with the stream it was issued on -- main, second,
weight-gradient (create_step_streams) or other.  The written file holds the list's length, SHA-256 and per-(call, stream)
counts; --calls-out keeps the lists themselves, --tensors the hashed tensors (FILE.json.pt), --compare checks three runs.
usage: python tools/step_digest.py [--train OTHER_TRAIN.py] [--out FILE.json [--tensors]] [--calls-out FILE.json] [--cases a,b]
       python tools/step_digest.py --compare PARENT_A.json PARENT_B.json NEW.json"""
import argparse
import collections
import hashlib
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BASE = dict(conf_thresh=0.05, conf_mode="pixelwise", mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all",
            maskclip_consistency_lambda=[0.1, 0])
OHEM = dict(criterion=dict(name="OHEM", kwargs=dict(ignore_index=255, thresh=0.7, min_kept=64)))
WEIGHT = [0.5 + 0.05 * i for i in range(21)]
# name -> (step, cfg on top of BASE, extras: teacher / fp_masks)
CASES = {
    "pixelwise_mean_all": ("semivl", {}, ()),
    "pixelavg_mean_valid": ("semivl", dict(conf_mode="pixelavg", mcc_loss_reduce="mean_valid"), ()),
    "pixelratio_mean": ("semivl", dict(conf_mode="pixelratio", mcc_loss_reduce="mean"), ()),
    "unguided": ("semivl", dict(maskclip_consistency_lambda=0), ()),
    "ohem": ("semivl", OHEM, ()),
    "celoss_smoothing_weight": ("semivl", dict(criterion=dict(name="CELoss", kwargs=dict(label_smoothing=0.1, weight=WEIGHT))), ()),
    "no_fuse_upsample_loss": ("semivl", dict(fuse_upsample_loss=False), ()),
    "no_overlap_streams": ("semivl", dict(overlap_streams=False), ()),
    "mean_teacher_labels": ("semivl", {}, ("teacher",)),
    "injected_fp_masks": ("semivl", {}, ("fp_masks",)),
    "supervised": ("supervised", {}, ()),
    "supervised_ohem": ("supervised", OHEM, ()),
    "supervised_weight": ("supervised", dict(criterion=dict(name="CELoss", kwargs=dict(weight=WEIGHT))), ()),
}


def load_train(path):
    """semivl_amd.train, or another version of the file standing in for it (nothing else in the package imports it)."""
    if path:
        spec = importlib.util.spec_from_file_location("semivl_amd.train", path)
        sys.modules["semivl_amd.train"] = mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    import semivl_amd.train as T
    return T


def sha(t):
    t = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


class CallLog:
    """Wraps lib.check for the duration of a step: (call, stream) in issue order."""

    def __init__(self, L, streams):
        self.L, self.calls = L, []
        self.names = {s_.cuda_stream: n_ for n_, s_ in zip(("main", "second", "weight-gradient"), streams)}

    def __enter__(self):
        self.check = self.L.check

        def check(rc, what=""):
            self.calls.append(f"{what}@{self.names.get(torch.cuda.current_stream().cuda_stream, 'other')}")
            return self.check(rc, what)
        self.L.check = check
        return self

    def __exit__(self, *exc):
        self.L.check = self.check


def run_case(T, name, dev):
    from golden_util import build_hip, fixture_batch, fixture_fp_masks, fixture_state, load_fixture
    import semivl_amd.lib as L
    from semivl_amd.ema import EmaTeacher
    from semivl_amd.synthetic import exp40_cfg
    step, over, extras = CASES[name]
    z, c = load_fixture("tiny")
    model = build_hip(c)
    model.load_state_dict(fixture_state(z, c, model), strict=True)
    model.to(dev)
    opt = T.FusedAdamW(model, exp40_cfg()["optimizer"], ema_decay=0.99)
    kw = dict(optimizer=opt, return_aux=True, teacher=EmaTeacher(model, opt) if "teacher" in extras else None)
    if "fp_masks" in extras:
        kw["fp_masks"] = [m.to(dev) for m in fixture_fp_masks(z, c)]
    host = fixture_batch(z, c)
    torch.manual_seed(0)        # the feature-dropout masks a step draws itself follow torch's generator
    log = CallLog(L, T.create_step_streams(dev))
    for it in (1, 2):
        batch = {k: v.clone().to(dev) for k, v in host.items()}    # (the semivl step cuts img_s1 / img_s2 in place)
        with log:
            if step == "semivl":
                loss, aux = T.semivl_train_step(model, batch, it, 10, dict(BASE, **over), **kw)
            else:
                loss, aux = T.supervised_train_step(model, dict(img_x=batch["img_x"], mask_x=batch["mask_x"]), it, 10,
                                                    dict(BASE, **over), **kw)
        torch.cuda.synchronize()
    out = {"loss": loss, "opt.p": opt.p, "opt.g": opt.g, "opt.ema": opt.ema}
    out.update({"aux." + k: v for k, v in aux.items()})
    digests = {k: (sha(v) if torch.is_tensor(v) else repr(v)) for k, v in sorted(out.items())}
    values = {k: v.detach().cpu() for k, v in out.items() if torch.is_tensor(v)}
    res = dict(upsample_in_loss=aux["upsample_in_loss"], digests=digests, n_calls=len(log.calls),
               calls_sha256=hashlib.sha256("\n".join(log.calls).encode()).hexdigest(),
               call_counts=dict(sorted(collections.Counter(log.calls).items())))
    return res, log.calls, values


def compare(paths):
    """PARENT_A PARENT_B NEW: the call lists must be identical in all three; a tensor the two parent runs agree on bit for bit
    must have the same bits in the new run; for one they do not, max |new - parent| <= max |parent_a - parent_b| (needs the
    tensors: FILE.json.pt next to each file, written by --out --tensors)."""
    runs = [json.load(open(p)) for p in paths]
    a, b, n = (r["cases"] for r in runs)
    bad, loose = [], 0
    for case in a:
        for key in ("n_calls", "calls_sha256", "call_counts", "upsample_in_loss"):
            if not (a[case][key] == b[case][key] == n[case][key]):
                bad.append(f"{case}: {key} differs")
        for k, d in a[case]["digests"].items():
            if d == b[case]["digests"][k]:
                if n[case]["digests"].get(k) != d:
                    bad.append(f"{case}: {k} differs from the two parent runs, which agree")
                continue
            loose += 1
            ta, tb, tn = (torch.load(p + ".pt")[case][k].double() for p in paths)
            spread, err = (ta - tb).abs().max().item(), min((tn - ta).abs().max().item(), (tn - tb).abs().max().item())
            print(f"{case}: {k} is not reproducible run to run: parent spread {spread:.3e}, new - parent {err:.3e}")
            if not err <= spread:
                bad.append(f"{case}: {k} new - parent {err:.3e} > parent spread {spread:.3e}")
    ups = {c_["upsample_in_loss"] for c_ in n.values()}
    if len(n) == len(CASES) and ups != {True, False}:
        bad.append(f"upsample_in_loss takes only {ups}")
    print("\n".join(bad) if bad else f"{len(a)} cases: call lists identical in all three runs; {loose} tensors differ between "
          f"the two parent runs (held to that spread), all others equal bit for bit in all three")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", default=None, help="another version of semivl_amd/train.py to run instead of the package's")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tensors", action="store_true", help="with --out: also keep the hashed tensors, in FILE.json.pt")
    ap.add_argument("--calls-out", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--compare", nargs=3, default=None)
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare)
    T = load_train(a.train)
    dev = torch.device("cuda:0")
    res, calls, values = {}, {}, {}
    for name in a.cases.split(","):
        res[name], calls[name], values[name] = run_case(T, name, dev)
        print(name, "upsample_in_loss", res[name]["upsample_in_loss"], "calls", res[name]["n_calls"], flush=True)
    out = dict(device=torch.cuda.get_device_name(0), cases=res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        if a.tensors:
            torch.save(values, a.out + ".pt")
    if a.calls_out:
        with open(a.calls_out, "w") as f:
            json.dump(calls, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
