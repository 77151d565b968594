"""The device-free parts of semivl_amd/optim.py: the arena's layout arithmetic, FusedSGD's two schedules through the shared
lr staging, and that FusedAdamW and FusedSGD share ONE base instead of carrying copies of it."""
import pytest
import torch


def test_arena_layout_pads_every_segment_to_four_floats():
    from semivl_amd.optim import arena_layout
    offs, total = arena_layout([5, 1000, 77, 4096, 4, 1])
    assert offs == [0, 8, 1008, 1088, 5184, 5188] and total == 5192
    assert arena_layout([]) == ([], 0)


LR, LR_MULTI = 1e-3, 10.0


def _sgd_stub(original):
    """Only what poly_lr reads, on the CPU (tests/test_host_logic.py::test_warmup_then_poly_lr's style)."""
    from semivl_amd.optim import FusedSGD

    class _O(FusedSGD):
        def __init__(self):
            self.groups = [dict(initial_lr=LR, lr=LR, group=0), dict(initial_lr=LR * LR_MULTI, lr=LR * LR_MULTI, group=1),
                           dict(initial_lr=LR * 0.01, lr=LR * 0.01, group=0)]
            self._lr_host, self.seg_lr, self._lr_evt = torch.zeros(3), torch.zeros(3), None
            self._members = [[], []] if original else None
            if original:
                self.lr, self.lr_multi, self._pg = LR, LR_MULTI, [dict(lr=LR), dict(lr=LR * LR_MULTI)]
    return _O()


@pytest.mark.parametrize("iters", [5, 50])
def test_sgd_poly_lr_mmcv_mode(iters):
    o = _sgd_stub(original=False)
    o.poly_lr(iters, 100, warmup_iters=10, warmup_ratio=1e-6)
    f = 1 - (1 - iters / 10) * (1 - 1e-6) if iters < 10 else (1 - iters / 100) ** 0.9       # semivl.py:339-345
    want = [g["initial_lr"] * f for g in o.groups]
    assert [g["lr"] for g in o.groups] == want and o._lr_factor == f and o.param_groups is o.groups
    assert torch.equal(o.seg_lr, torch.tensor(want, dtype=torch.float32))


@pytest.mark.parametrize("iters", [5, 50])
def test_sgd_poly_lr_original_mode(iters):
    from semivl_amd.optim import sgd_original_lr
    o = _sgd_stub(original=True)
    o.poly_lr(iters, 100, warmup_iters=10, warmup_ratio=1e-6)
    lrs = sgd_original_lr(LR, LR_MULTI, iters, 100, 10, 1e-6)
    assert [g["lr"] for g in o.param_groups] == list(lrs) and len(o.param_groups) == 2
    want = [lrs[g["group"]] for g in o.groups]
    assert [g["lr"] for g in o.groups] == want and [g["initial_lr"] for g in o.groups] == [LR, LR * LR_MULTI, LR * 0.01]
    assert torch.equal(o.seg_lr, torch.tensor(want, dtype=torch.float32))


def test_both_optimizers_share_one_base():
    from semivl_amd import optim, train
    base = optim.ArenaOptimizer
    assert optim.FusedAdamW.__bases__ == (base,) and optim.FusedSGD.__bases__ == (base,)
    for cls in (optim.FusedAdamW, optim.FusedSGD):
        for name in ("zero_grad", "_fold_autograd_grads", "_stage_lr", "step"):
            assert name not in vars(cls) and name in vars(base), (cls.__name__, name)
    assert "poly_lr" not in vars(optim.FusedAdamW) and "state_dict" not in vars(optim.FusedAdamW)
    for name in ("FusedAdamW", "FusedSGD", "build_optimizer", "optimizer_from_cfg", "mmcv_param_groups", "sgd_original_groups",
                 "sgd_original_lr"):
        assert getattr(train, name) is getattr(optim, name), name
