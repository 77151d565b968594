"""Host logic of semivl_amd.trainer (no GPU): cfg['trainer'] validation, the epoch / iters arithmetic and the evaluation
schedule of semivl.py:181-185,408, the per-epoch seed mix, save_checkpoint(extra=) and the metrics.jsonl writer."""
import json
import math
import random

import numpy as np
import pytest
import torch

from semivl_amd import trainer as T


def test_trainer_defaults():
    want = dict(seed=0, log_interval=100, debug_panels=True, save_latest=True, workers=4, prefetch=2)
    assert T.trainer_from_cfg({}) == want
    assert T.trainer_from_cfg(dict(trainer={})) == want
    got = T.trainer_from_cfg(dict(trainer=dict(seed=7, log_interval=1, debug_panels=False, workers=np.int64(2))))
    assert got == dict(want, seed=7, log_interval=1, debug_panels=False, workers=2) and type(got["workers"]) is int


@pytest.mark.parametrize("spec,word", [
    ([1, 2], "expected a dict"), ("fast", "expected a dict"), (None, "expected a dict"),
    (dict(sead=1), "'sead'"), (dict(log_every=5), "'log_every'"),
    (dict(seed=True), "seed"), (dict(seed=1.0), "seed"), (dict(seed="3"), "seed"), (dict(seed=-1), "seed"),
    (dict(seed=2 ** 31), "seed"),
    (dict(log_interval=0), "log_interval"), (dict(log_interval=False), "log_interval"), (dict(log_interval=2.5), "log_interval"),
    (dict(workers=0), "workers"), (dict(workers=True), "workers"), (dict(workers=None), "workers"),
    (dict(prefetch=0), "prefetch"), (dict(prefetch=-3), "prefetch"), (dict(prefetch=True), "prefetch"),
    (dict(debug_panels=1), "debug_panels"), (dict(debug_panels="yes"), "debug_panels"), (dict(debug_panels=None), "debug_panels"),
    (dict(save_latest=0), "save_latest"), (dict(save_latest="no"), "save_latest"),
])
def test_trainer_refusals_name_the_offender(spec, word):
    with pytest.raises(ValueError, match="trainer: .*" + word):
        T.trainer_from_cfg(dict(trainer=spec))


@pytest.mark.parametrize("iters,steps", [(1, 1), (1, 4), (4, 4), (5, 4), (8, 4), (9, 4), (40000, 662), (40000, 1323), (7, 3)])
def test_epochs_from_iters(iters, steps):
    """semivl.py:181-185: epochs = ceil(iters / len(loader)), total_iters = len(loader) * epochs."""
    epochs, total = T.schedule_from_cfg(dict(iters=iters, epochs=None), steps)
    assert epochs == math.ceil(iters / steps) and total == steps * epochs and total >= iters and total - iters < steps
    assert T.schedule_from_cfg(dict(iters=iters), steps) == (epochs, total)
    assert T.schedule_from_cfg(dict(epochs=epochs), steps) == (epochs, total)
    assert T.schedule_from_cfg(dict(iters=iters, scheduler_max_iters=total), steps) == (epochs, total)
    with pytest.raises(ValueError, match="scheduler_max_iters"):
        T.schedule_from_cfg(dict(iters=iters, scheduler_max_iters=total - 1), steps)


def test_schedule_refusals():
    with pytest.raises(ValueError, match="both 'iters' and 'epochs'"):
        T.schedule_from_cfg(dict(iters=10, epochs=2), 4)
    with pytest.raises(ValueError, match="needs 'iters'"):
        T.schedule_from_cfg({}, 4)
    with pytest.raises(ValueError, match="steps per epoch"):
        T.schedule_from_cfg(dict(iters=10), 0)
    for bad in (0, -1, True, 2.5, "8"):
        with pytest.raises(ValueError, match="'iters'"):
            T.schedule_from_cfg(dict(iters=bad), 4)
        with pytest.raises(ValueError, match="'epochs'"):
            T.schedule_from_cfg(dict(epochs=bad), 4)


def test_eval_schedule():
    """semivl.py:408: epoch % eval_every_n_epochs == 0 or epoch == epochs - 1."""
    for epochs in (1, 2, 5, 8):
        for every in (1, 2, 3, 10):
            due = [e for e in range(epochs) if T.eval_due(e, epochs, every)]
            assert due == sorted(set(range(0, epochs, every)) | {epochs - 1})
    assert [T.eval_due(e, 3) for e in range(3)] == [True] * 3


def test_log_points():
    steps, every = 4, 3
    pts = [(e * steps + i) for e in range(3) for i in range(steps) if T.is_log_point(e * steps + i, i, steps, every)]
    assert pts == [0, 3, 6, 7, 9, 11]       # iters % 3 == 0, and every epoch's last step


def test_seed_mix_is_distinct_and_stable():
    seen = {}
    for seed in (0, 1, 2, 12345):
        for epoch in range(50):
            for rank in range(8):
                s = T.epoch_seed(seed, epoch, rank)
                assert 0 <= s < 2 ** 32 and s == T.epoch_seed(seed, epoch, rank)
                assert s not in seen, (seen[s], (seed, epoch, rank))
                seen[s] = (seed, epoch, rank)
    assert T.epoch_seed(3, 4, 5) == ((3 * 1000003 + 4) * 1009 + 5) % 2 ** 32
    assert T.epoch_seed(2 ** 31 - 1, 10 ** 6, 1008) < 2 ** 32


def test_seed_epoch_seeds_all_three_generators():
    def draws():
        return random.random(), float(np.random.rand()), float(torch.rand(1)), torch.initial_seed()
    s = T.seed_epoch(5, 2, 1)
    a = draws()
    random.random(), np.random.rand(), torch.rand(3)        # history ...
    assert T.seed_epoch(5, 2, 1) == s
    assert draws() == a                                     # ... does not matter
    assert a[3] == s
    T.seed_epoch(5, 3, 1)
    b = draws()
    assert all(x != y for x, y in zip(a, b))


def test_save_checkpoint_extra_round_trips(tmp_path):
    from semivl_amd.checkpoint import load_checkpoint, save_checkpoint
    torch.manual_seed(0)
    model, other = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    plain = save_checkpoint(str(tmp_path / "plain.pth"), model, None, 4)
    assert sorted(plain) == ["epoch", "model", "optimizer"]
    assert sorted(torch.load(tmp_path / "plain.pth")) == ["epoch", "model", "optimizer"]         # files without it: unchanged
    assert sorted(save_checkpoint(str(tmp_path / "none.pth"), model, None, 4, extra=None)) == ["epoch", "model", "optimizer"]
    extra = dict(previous_best=61.25, seed=3, total_iters=8)
    save_checkpoint(str(tmp_path / "x.pth"), model, None, 4, ema_model=other, extra=extra)
    ck = torch.load(tmp_path / "x.pth")
    assert sorted(ck) == sorted(["epoch", "model", "optimizer", "ema_model", "previous_best", "seed", "total_iters"])
    assert {k: ck[k] for k in extra} == extra and ck["epoch"] == 4
    assert all(torch.equal(ck["model"][k], plain["model"][k]) for k in plain["model"])
    fresh = torch.nn.Linear(3, 2)
    assert load_checkpoint(str(tmp_path / "x.pth"), fresh) == 4 and torch.equal(fresh.weight, model.weight)
    assert load_checkpoint(str(tmp_path / "x.pth"), fresh, ema=True) == 4 and torch.equal(fresh.weight, other.weight)
    for key in ("model", "optimizer", "epoch", "ema_model"):
        with pytest.raises(ValueError, match=repr(key)):
            save_checkpoint(str(tmp_path / "bad.pth"), model, None, 4, extra={key: 1})
    with pytest.raises(ValueError, match="extra must be a dict"):
        save_checkpoint(str(tmp_path / "bad.pth"), model, None, 4, extra=[("seed", 1)])
    assert not (tmp_path / "bad.pth").exists()


def test_metrics_writer(tmp_path):
    path = tmp_path / "run" / "metrics.jsonl"
    w = T.MetricsWriter(path)
    w.write("train", epoch=0, iters=3, **{"train/loss_all": np.float64(0.5), "train/iter_time": 0.01})
    w.write("eval", epoch=0, **{"eval/mIoU": np.float32(12.5), "eval/iou_class": np.array([1.0, float("nan"), 3.0])},
            nested=dict(hist=np.arange(3), flag=np.bool_(True), n=np.int64(4)))
    T.MetricsWriter(path).write("train", epoch=1, iters=7, inf=float("inf"))          # a resumed run appends
    lines = path.read_text().splitlines()
    assert len(lines) == 3 and all(json.loads(l) for l in lines)
    recs = T.read_metrics(path)
    assert recs[0] == {"kind": "train", "epoch": 0, "iters": 3, "train/loss_all": 0.5, "train/iter_time": 0.01}
    assert recs[1]["eval/mIoU"] == 12.5 and recs[1]["eval/iou_class"] == [1.0, None, 3.0]
    assert recs[1]["nested"] == {"hist": [0, 1, 2], "flag": True, "n": 4}
    assert recs[2] == {"kind": "train", "epoch": 1, "iters": 7, "inf": None}


def test_default_id_paths():
    assert T.default_id_paths(dict(dataset="pascal", split="92")) == ("splits/pascal/92/labeled.txt", "splits/pascal/92/unlabeled.txt")


def test_train_refuses_the_cfg_before_anything_is_built(tmp_path):
    for cfg, word in ((dict(trainer=dict(sead=1)), "'sead'"), (dict(method="fixmatch"), "method 'fixmatch'"),
                      (dict(palette=[1, 2]), "palette"), (dict(eval_every_n_epochs=0), "eval_every_n_epochs")):
        with pytest.raises(ValueError, match=word):
            T.train(cfg, str(tmp_path / "out"), "no_such_l.txt", "no_such_u.txt")
    assert not (tmp_path / "out").exists()
