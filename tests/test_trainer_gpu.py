"""GPU: semivl_amd.trainer.train and `python -m semivl_amd.tools.train` on a dataset of seventeen small PNG images (6
labelled, 8 unlabelled, 3 validation; batch 2 = 4 steps per epoch) and the tiny product VLM of tests/test_evalreport_gpu.py.
Every comparison is exact: the logged means are the float64 means of a hand-written loop's per-step fp32 losses, final
parameters are that loop's bit for bit, a run stopped after epoch 0 and resumed equals the straight run, the logged mIoU is
`evaluate` on the reloaded latest.pth."""
import copy
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP = 128
NAMES = ("loss_all", "loss_x", "loss_s1", "loss_s2", "loss_fp")


def _write_images(root, tag, n, seed):
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    ids = []
    for i in range(n):
        h, w = 100 + 4 * (i % 3), 120 - 6 * (i % 2)
        img = torch.nn.functional.avg_pool2d(torch.randn(1, 3, h, w, generator=g), 9, stride=1, padding=4)[0]
        img = ((img / img.std()) * 60 + 128).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
        lbl = torch.randint(0, 21, (h // 8 + 1, w // 8 + 1), generator=g).repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w]
        lbl[:, :5] = 255
        Image.fromarray(img).save(root / "JPEGImages" / f"{tag}{i}.png")
        Image.fromarray(lbl.to(torch.uint8).numpy()).save(root / "SegmentationClass" / f"{tag}{i}.png")
        ids.append(f"JPEGImages/{tag}{i}.png SegmentationClass/{tag}{i}.png")
    return ids


def _dataset(tmp):
    """The images, the three split files and the config of an unguided run (2 epochs of 4 steps)."""
    from semivl_amd.model.builder import builtin_model_cfg
    root = tmp / "data"
    os.makedirs(root / "JPEGImages")
    os.makedirs(root / "SegmentationClass")
    split = tmp / "splits" / "pascal" / "tiny"
    os.makedirs(split)
    for name, tag, n, seed in (("labeled", "l", 6, 1), ("unlabeled", "u", 8, 2), ("val", "v", 3, 3)):
        (split / f"{name}.txt").write_text("\n".join(_write_images(root, tag, n, seed)) + "\n")
    m = copy.deepcopy(builtin_model_cfg("vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb"))["model"]
    m["backbone"].update(img_size=(CROP, CROP), embed_dims=64, num_layers=3, num_heads=1, out_indices=[0, 1, 3])
    m["decode_head"].update(img_size=CROP, num_classes=21, text_channels=32, up_channels=(32, 16), skip_in_channels=(64, 64),
                            skip_channels=(16, 16), num_heads=1, channels=32)
    cfg = dict(dataset="pascal", split="tiny", data_root=str(root), val_id_path=str(split / "val.txt"), nclass=21,
               crop_size=CROP, scale_ratio_range=[0.5, 2.0], batch_size=2, iters=8, epochs=None, method="semivl",
               model="mmseg.vlm-vlg-aspp-s2p4-sk04-ftap-mcvitb", text_embedding_variant="single", mcc_text="concept4_single",
               pl_text="single", disable_dropout=True, fp_rate=0.5, allow_random_init=True, pretrained=None,
               model_args=dict(backbone=m["backbone"], decode_head=m["decode_head"], pretrained=None),
               clip_encoder=None, maskclip_consistency_lambda=0, conf_thresh=0.0, conf_mode="pixelwise",
               mcc_conf_thresh=0.9, mcc_loss_reduce="mean_all", criterion=dict(name="CELoss", kwargs=dict(ignore_index=255)),
               optimizer=dict(type="AdamW", lr=1e-3, weight_decay=0.01), eval_mode="original",
               trainer=dict(seed=5, log_interval=3, workers=2))
    return cfg, str(split / "labeled.txt"), str(split / "unlabeled.txt")


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _hand_loop(cfg, lab, unl, dev, epochs):
    """The loop of INTEGRATION.md written out: StepLoader + semivl_train_step (or LabeledLoader + supervised_train_step)
    with the trainer's seeding; -> (per-step fp32 loss vectors on the host, the optimizer)."""
    from semivl_amd import trainer as T
    from semivl_amd.data import GpuAugmenter, LabeledLoader, SemiDataset, StepLoader
    from semivl_amd.model.builder import build_model
    from semivl_amd.optim import optimizer_from_cfg
    from semivl_amd.train import semivl_train_step, supervised_train_step
    seed = cfg["trainer"]["seed"]
    T.seed_epoch(seed, 0, 0)
    model = build_model(cfg).to(dev)
    opt = optimizer_from_cfg(model, cfg)
    aug = GpuAugmenter.from_cfg(cfg, device=dev)
    semi = cfg["method"] == "semivl"
    if semi:
        set_u = SemiDataset(cfg, "train_u", id_path=unl)
        set_l = SemiDataset(cfg, "train_l", id_path=lab, nsample=len(set_u.ids))
    else:
        set_l = SemiDataset(cfg, "train_l", id_path=lab)
    losses, steps = [], None
    for epoch in range(epochs):
        T.seed_epoch(seed, epoch, 0)
        loader = (StepLoader(set_l, set_u, aug, cfg["batch_size"], epoch=epoch, workers=2) if semi else
                  LabeledLoader(set_l, aug, cfg["batch_size"], epoch=epoch, workers=2))
        steps = len(loader)
        for i, batch in enumerate(loader):
            step = semivl_train_step if semi else supervised_train_step
            losses.append(step(model, batch, epoch * steps + i, steps * epochs, cfg, optimizer=opt).clone())
    torch.cuda.synchronize()
    return [l.cpu() for l in losses], opt, model, steps


def _segment_means(losses, points):
    """float64 sums in step order over the steps between log points, divided by their count -- what LossMeter holds."""
    out, start = [], 0
    for p in points:
        s = np.zeros(losses[0].numel(), np.float64)
        for l in losses[start:p + 1]:
            s += l.numpy().astype(np.float64)
        out.append(s / (p + 1 - start))
        start = p + 1
    return out


def test_two_epoch_run_equals_the_hand_written_loop(dev, tmp_path, capsys):
    from PIL import Image
    from semivl_amd import trainer as T
    from semivl_amd.checkpoint import load_checkpoint
    from semivl_amd.data import GpuAugmenter, ValLoader
    from semivl_amd.evaluate import evaluate
    from semivl_amd.model.builder import build_model
    cfg, lab, unl = _dataset(tmp_path)
    out = tmp_path / "run"
    res = T.train(cfg, str(out), lab, unl)
    text = capsys.readouterr().out
    assert res["epochs_run"] == 2 and res["epochs"] == 2 and res["total_iters"] == 8 and res["teacher"] is None
    # files
    want = {"config.yaml", "train.log", "metrics.jsonl", "latest.pth", "debug"} | ({"best.pth"} if res["best"] > 0 else set())
    assert set(os.listdir(out)) == want and res["best"] > 0
    assert sorted(os.listdir(out / "debug")) == [f"{it:07d}_0-{b}.png" for it in (0, 4) for b in (0, 1)]
    with Image.open(out / "debug" / "0000004_0-1.png") as im:
        assert im.mode == "RGB" and im.size == (4 * CROP, 3 * CROP)          # unguided: three rows
    import yaml
    assert yaml.load(open(out / "config.yaml"), Loader=yaml.Loader) == cfg
    log_lines = (out / "train.log").read_text().splitlines()
    assert len(log_lines) > 10 and all(line in text for line in log_lines)
    # the hand-written loop: means and parameters
    losses, opt, _, steps = _hand_loop(cfg, lab, unl, dev, 2)
    assert steps == 4 and len(losses) == 8
    recs = T.read_metrics(out / "metrics.jsonl")
    train = [r for r in recs if r["kind"] == "train"]
    assert [r["iters"] for r in train] == [0, 3, 6, 7] and [r["steps"] for r in train] == [1, 3, 3, 1]
    for r, mean in zip(train, _segment_means(losses, [0, 3, 6, 7])):
        for k, name in enumerate(NAMES):
            print(r["iters"], name, r["train/" + name], mean[k])
            assert r["train/" + name] == mean[k], (r["iters"], name)
        assert "train/loss_mc_s1" not in r and r["train/iter_time"] > 0
    assert _bits(res["optimizer"].p, opt.p)
    assert f"Iters: 3 train/iter_time: {train[1]['train/iter_time']:.3f}, train/loss_all: {train[1]['train/loss_all']:.3f}, " in text
    assert "Train for 2 epochs / 8 iterations." in text and "===========> Epoch: 1, LR: " in text
    # evaluation: the logged mIoU is evaluate() on the reloaded latest.pth
    ev = [r for r in recs if r["kind"] == "eval"]
    assert [r["epoch"] for r in ev] == [0, 1] and ev[1]["previous_best"] == res["best"] == max(r["eval/mIoU"] for r in ev)
    model = build_model(cfg).to(dev)
    assert load_checkpoint(str(out / "latest.pth"), model) == 1
    miou, iou = evaluate(model, ValLoader(cfg, GpuAugmenter.from_cfg(cfg, device=dev)), "original", cfg)
    assert ev[1]["eval/mIoU"] == miou == res["report"]["mIoU"] and ev[1]["eval/iou_class"] == iou.tolist()
    assert "***** Evaluation original ***** >>>> MeanIoU: {:.2f}\n".format(miou) in text
    ck = torch.load(out / "latest.pth")
    assert ck["previous_best"] == res["best"] and ck["seed"] == 5 and ck["total_iters"] == 8 and ck["epoch"] == 1


def _state(res):
    opt = res["optimizer"]
    out = {"p": opt.p, "ema": opt.ema}
    for name in ("m", "v"):
        if getattr(opt, name, None) is not None:
            out[name] = getattr(opt, name)
    out.update({"buf/" + k: v for k, v in res["model"].named_buffers()})
    out.update({"tbuf/" + k: v for k, v in res["teacher"].model.named_buffers()})
    return {k: v.detach().clone() for k, v in out.items()}


def test_resumed_run_continues_bit_for_bit(dev, tmp_path):
    from semivl_amd import trainer as T
    cfg, lab, unl = _dataset(tmp_path)
    cfg = dict(cfg, ema=dict(decay=0.9), optimizer_config=dict(grad_clip=dict(max_norm=1.0)),
               pl_monitor=dict(conf_bins=10, gt=True), trainer=dict(seed=5, log_interval=3, workers=2, debug_panels=False))
    runs = {}
    for tag in ("a", "a2", "b"):
        steps = {}
        rec = lambda it, l, steps=steps: steps.__setitem__(it, l.clone())
        if tag == "b":
            first = T.train(cfg, str(tmp_path / tag), lab, unl, stop_after_epoch=0, on_step=rec)
            assert first["epochs_run"] == 1 and sorted(steps) == [0, 1, 2, 3]
            assert torch.load(tmp_path / tag / "latest.pth")["epoch"] == 0
            del first
            res = T.train(cfg, str(tmp_path / tag), lab, unl, resume=str(tmp_path / tag / "latest.pth"), on_step=rec)
            assert res["epochs_run"] == 1
        else:
            res = T.train(cfg, str(tmp_path / tag), lab, unl, on_step=rec)
            assert res["epochs_run"] == 2
        assert sorted(steps) == list(range(8)) and res["teacher"] is not None and res["optimizer"].grad_clip is not None
        torch.cuda.synchronize()
        runs[tag] = (_state(res), {k: v.cpu() for k, v in steps.items()}, res["best"], res["report"])
        del res
    (sa, la, ba, ra), (sa2, la2, ba2, _), (sb, lb, bb, rb) = runs["a"], runs["a2"], runs["b"]
    assert sorted(sa) == sorted(sb) and {"p", "ema", "m", "v"} <= set(sa)

    def diff(x, y):
        assert torch.isfinite(x.double()).all() and torch.isfinite(y.double()).all()
        return float((x.double() - y.double()).abs().max()) if x.numel() else 0.0
    # two identical straight runs: any difference between them is reported, and bounds what the resumed run may differ by
    base = {k: diff(sa[k], sa2[k]) for k in sa}
    base_l = {it: diff(la[it], la2[it]) for it in la}
    print("straight run vs straight run: max |difference|", max(base.values()), max(base_l.values()), abs(ba - ba2))
    for k in sa:
        assert diff(sa[k], sb[k]) <= base[k], k
        if base[k] == 0.0:
            assert _bits(sa[k], sb[k]), k
    for it in range(4, 8):          # the epoch-1 step losses
        assert diff(la[it], lb[it]) <= base_l[it], it
        if base_l[it] == 0.0:
            assert _bits(la[it], lb[it]), it
    assert abs(ba - bb) <= abs(ba - ba2) and abs(ra["ema_mIoU"] - rb["ema_mIoU"]) <= abs(ba - ba2)
    assert not _bits(sa["p"], sa["ema"])
    # the metrics of the resumed run continue the file; the monitor reported at every log point
    recs = T.read_metrics(tmp_path / "b" / "metrics.jsonl")
    train = [r for r in recs if r["kind"] == "train"]
    assert [r["iters"] for r in train] == [0, 3, 6, 7]
    assert all("pl_monitor" in r and r["pl_monitor"]["steps"] == r["steps"] and "pl_miou" in r["pl_monitor"] for r in train)
    assert all("train/grad_norm" in r and r["train/grad_nonfinite"] == 0.0 for r in train)
    assert [r["epoch"] for r in recs if r["kind"] == "eval"] == [0, 1] and all("eval/ema_mIoU" in r for r in recs if r["kind"] == "eval")
    # a resume under another schedule or seed is refused
    for other, word in ((dict(cfg, iters=12), "total_iters"), (dict(cfg, trainer=dict(cfg["trainer"], seed=6)), "seed")):
        with pytest.raises(ValueError, match=word):
            T.train(other, str(tmp_path / "c"), lab, unl, resume=str(tmp_path / "b" / "latest.pth"))


def test_supervised_method_equals_its_hand_written_loop(dev, tmp_path):
    from semivl_amd import trainer as T
    cfg, lab, unl = _dataset(tmp_path)
    cfg = dict(cfg, method="supervised", iters=None, epochs=1, trainer=dict(seed=2, log_interval=2))
    res = T.train(cfg, str(tmp_path / "sup"), lab, unl)
    assert res["epochs_run"] == 1 and res["total_iters"] == 3 and not os.path.exists(tmp_path / "sup" / "debug")
    losses, opt, _, steps = _hand_loop(cfg, lab, unl, dev, 1)
    assert steps == 3 and all(l.numel() == 1 for l in losses)
    train = [r for r in T.read_metrics(tmp_path / "sup" / "metrics.jsonl") if r["kind"] == "train"]
    assert [r["iters"] for r in train] == [0, 2]
    for r, mean in zip(train, _segment_means(losses, [0, 2])):
        assert r["train/loss_all"] == mean[0] and set(r) == {"kind", "epoch", "iters", "steps", "train/iter_time", "train/loss_all"}
    assert _bits(res["optimizer"].p, opt.p)
    assert os.path.exists(tmp_path / "sup" / "latest.pth")


def _tiny_clip_cfg(tmp):
    """configs/_base_/models/mcvit16.py under `tmp`: the guidance encoder at the tiny model's dimensions (load_model_cfg
    reads a file of the working directory first)."""
    from semivl_amd.model.builder import builtin_model_cfg
    bb = copy.deepcopy(builtin_model_cfg("mcvit16"))["backbone"]
    bb.update(img_size=(CROP, CROP), embed_dims=64, num_layers=3, num_heads=1)
    bb.pop("pretrained", None)
    os.makedirs(tmp / "configs" / "_base_" / "models")
    (tmp / "configs" / "_base_" / "models" / "mcvit16.py").write_text(f"img_size = {CROP}\nbackbone = {bb!r}\n")


def test_train_tool_guided_with_resume(dev, tmp_path, capsys, monkeypatch):
    import yaml
    from PIL import Image
    from semivl_amd import trainer as T
    from semivl_amd.tools.train import main
    cfg, lab, unl = _dataset(tmp_path)
    cfg.update(clip_encoder="mcvit16", maskclip_consistency_lambda=[0.1, 0], iters=4, eval_report=dict(metrics=["mIoU", "mAcc"]),
               palette=[0, 0, 0, 255, 0, 0, 0, 255, 0])
    _tiny_clip_cfg(tmp_path)
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.dump(cfg, f)
    monkeypatch.chdir(tmp_path)                 # the default id paths are splits/<dataset>/<split>/... of the working directory
    res = main(["--config", "cfg.yaml", "--save-path", "out"])
    text = capsys.readouterr().out
    assert res["epochs_run"] == 1 and res["total_iters"] == 4
    assert "Iters: 0 train/iter_time: " in text and "train/loss_mc_fp: " in text and "aAcc" in text
    assert "***** Evaluation original ***** >>>> MeanIoU: {:.2f}\n".format(res["report"]["mIoU"]) in text
    train = [r for r in T.read_metrics("out/metrics.jsonl") if r["kind"] == "train"]
    assert [r["iters"] for r in train] == [0, 3] and all("train/loss_mc_s1" in r for r in train)
    with Image.open("out/debug/0000000_0-0.png") as im:
        arr = np.array(im)
    assert arr.shape == (4 * CROP, 4 * CROP, 3) and (arr[3 * CROP:, :CROP] == 255).all()      # guided: four rows, a white slot
    colours = {tuple(c) for c in arr[CROP:3 * CROP].reshape(-1, 3).tolist()}
    assert colours <= {(0, 0, 0), (255, 0, 0), (0, 255, 0), (255, 255, 255)}                   # cfg['palette']: three colours
    # --resume (default file): the finished run has nothing left to do and says where it stands
    again = main(["--config", "cfg.yaml", "--save-path", "out", "--resume", "--labeled-id-path", lab, "--unlabeled-id-path", unl])
    text = capsys.readouterr().out
    assert again["epochs_run"] == 0 and again["best"] == res["best"] and "Load from checkpoint at epoch 0" in text
    assert _bits(again["optimizer"].p, res["optimizer"].p)
    cfg["iters"] = 8
    with open(tmp_path / "cfg8.yaml", "w") as f:
        yaml.dump(cfg, f)
    with pytest.raises(ValueError, match="total_iters"):
        main(["--config", "cfg8.yaml", "--save-path", "out", "--resume", "out/latest.pth"])


def _group_worker(port, tmp, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0",
                      GPU_MAX_HW_QUEUES="8", SVL_NO_WGRAD_STREAM="1")
    import pathlib
    import torch.distributed as dist
    from semivl_amd import trainer as T
    import test_trainer_gpu as me
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tmp = pathlib.Path(tmp)
    cfg, lab, unl = me._dataset(tmp)
    cfg = dict(cfg, iters=4, ema=dict(decay=0.9))
    plain = T.train(cfg, str(tmp / "plain"), lab, unl)
    p_plain, e_plain = plain["optimizer"].p.cpu().numpy(), plain["optimizer"].ema.cpu().numpy()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    grp = T.train(cfg, str(tmp / "group"), lab, unl)
    q.put(dict(plain=p_plain, group=grp["optimizer"].p.cpu().numpy(), ema_plain=e_plain, ema_group=grp["optimizer"].ema.cpu().numpy(),
               best=(plain["best"], grp["best"]), files=sorted(os.listdir(tmp / "group")),
               grad_scale=grp["optimizer"].grad_scale))
    dist.barrier()
    dist.destroy_process_group()


def test_run_under_a_one_rank_process_group(dev, tmp_path):
    """The trainer's distributed branch (GradAllReducer, broadcast_params, teacher.reset, the evaluator's and the monitor's
    all-reduces, the barrier after the checkpoint) under an initialised one-rank RCCL group: the identity, bit for bit."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_group_worker, args=(29900 + os.getpid() % 90, str(tmp_path), q))
    p.start()
    out = q.get(timeout=600)
    p.join(120)
    assert p.exitcode == 0
    assert np.array_equal(out["plain"], out["group"]) and np.array_equal(out["ema_plain"], out["ema_group"])
    assert out["best"][0] == out["best"][1] and out["grad_scale"] == 1.0
    assert {"latest.pth", "metrics.jsonl", "train.log", "config.yaml", "debug"} <= set(out["files"])
