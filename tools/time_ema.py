"""ms per training step with and without the mean teacher (semivl_amd/ema.py), same model, same optimizer (fused AdamW with
the EMA arena in both arms: what differs is who supplies the pseudo-labels and the teacher's buffer launch), split arithmetic
mode 6, the guided default.  Rows: `vlg` = VOC B = 16 labeled + 16 unlabeled images at 512^2 (exp-40 recipe) and `dlv3p` = the
DeepLabV3+ `ftap` ablation row on the same data, where the teacher moves the pseudo-label pass to the second stream.  The two
arms alternate in --rounds rounds of --warmup + --steps steps within one call; reported per arm: the median round's ms/step,
every round, and torch.cuda.max_memory_allocated.  Prints one JSON line at the end (profiles/ema_step_times.json).
usage: python tools/time_ema.py [--rows vlg,dlv3p] [--rounds R] [--steps N] [--warmup W] [--batch B]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

DLV3P = "mmseg.vlm-dlv3p-bn12-sk4-ftap-mcvitb"


def time_row(row, rounds, steps, warmup, batch_size, dev):
    from semivl_amd.ema import EmaTeacher
    from semivl_amd.model.builder import build_model
    from semivl_amd.optim import optimizer_from_cfg
    from semivl_amd.synthetic import exp40_cfg, synthetic_batch
    from semivl_amd.train import semivl_train_step
    cfg = exp40_cfg(batch_size, 512, 21, "pascal")
    if row == "dlv3p":
        cfg["model"] = DLV3P
    cfg["ema"] = dict(decay=0.996)
    torch.manual_seed(1234)
    model = build_model(cfg).to(dev)
    opt = optimizer_from_cfg(model, cfg)
    teacher = EmaTeacher.from_cfg(model, opt, cfg)
    batch = synthetic_batch(batch_size, 512, 21, seed=1234, device=dev)
    arms = {"no_teacher": None, "teacher": teacher}
    ms = {k: [] for k in arms}
    mem = {}
    it = 0
    for _ in range(rounds):
        for name, t in arms.items():
            torch.cuda.reset_peak_memory_stats()
            for _ in range(warmup):
                semivl_train_step(model, batch, it, 100000, cfg, optimizer=opt, teacher=t)
                it += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                semivl_train_step(model, batch, it, 100000, cfg, optimizer=opt, teacher=t)
                it += 1
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
            mem[name] = max(mem.get(name, 0), torch.cuda.max_memory_allocated())
            print(f"{row:6s} {name:10s} {ms[name][-1]:8.2f} ms/step  {2e3 * batch_size / ms[name][-1]:6.1f} img/s  peak "
                  f"{mem[name] / 2 ** 30:.2f} GiB", flush=True)
    del model, opt, teacher, arms
    torch.cuda.empty_cache()
    return {k: dict(ms_per_step=round(statistics.median(v), 2), rounds_ms=[round(x, 2) for x in v],
                    max_memory_allocated=mem[k]) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="vlg,dlv3p")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    from semivl_amd import ops
    dev = torch.device("cuda:0")
    ops.set_gemm_emulation(6)
    res = {row: time_row(row, a.rounds, a.steps, a.warmup, a.batch, dev) for row in a.rows.split(",")}
    print(json.dumps(dict(tool="time_ema", device=torch.cuda.get_device_name(0), batch=a.batch, crop=512, gemm_emulation=6,
                          optimizer="FusedAdamW + EMA arena (both arms)", ema=dict(decay=0.996, warmup=True), rounds=a.rounds,
                          steps=a.steps, warmup=a.warmup, rows=res)))


if __name__ == "__main__":
    main()
