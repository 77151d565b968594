"""CPU proof of tests/gradclip_ref.py (the float64 restatement of svl_grad_clip_f32 and its bound) against
torch.nn.utils.clip_grad_norm_, every accept / refuse / raise rule of grad_clip_from_cfg, and the optimizer_from_cfg paths
that run without a GPU."""
import math

import pytest
import torch

import gradclip_ref as R

SIZES = [7, 1, 130, 33, 4, 1025]          # tensors of unequal sizes: what clip_grad_norm_ walks, what the arena pads to 4


def _tensors(seed, dtype, kind="normal"):
    flat = R.values(kind, sum(SIZES), seed).to(dtype)
    return [t.clone() for t in flat.split(SIZES)]


def _arena(tensors):
    """The flat view the kernel reads: every tensor padded with zeros to a multiple of 4 floats (optim.arena_layout)."""
    from semivl_amd.optim import arena_layout
    offs, total = arena_layout([t.numel() for t in tensors])
    g = torch.zeros(total, dtype=tensors[0].dtype)
    for o, t in zip(offs, tensors):
        g[o:o + t.numel()] = t
    return g


@pytest.mark.parametrize("norm_type", [2.0, math.inf], ids=["l2", "max"])
@pytest.mark.parametrize("clip", ["live", "idle", "report"])
def test_restatement_equals_torch_in_float64(norm_type, clip):
    tensors = _tensors(3, torch.float64)
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in tensors]
    for p, t in zip(params, tensors):
        p.grad = t.clone()
    n0 = R.clip_ref(_arena(tensors), math.inf, norm_type)[0]
    max_norm = dict(live=0.37 * n0, idle=2.5 * n0, report=math.inf)[clip]
    got = float(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type))
    # (float64 inputs: max_norm is not an fp32 number here, so the restatement's own rounding of it is bypassed by hand)
    norm, _, _, flag = R.clip_ref(_arena(tensors), math.inf, norm_type)
    coef = min(max_norm / (norm + 1e-6), 1.0)
    assert abs(norm - got) <= 1e-12 * got and not flag
    assert (coef < 1.0) == (clip == "live")
    for p, t in zip(params, tensors):
        want = t * coef
        assert (p.grad - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # and through clip_ref with an fp32 max_norm, as the kernel gets it
    mn = R.f32(max_norm)
    _, coef32, scale, _ = R.clip_ref(_arena(tensors), mn, norm_type, gscale=0.5)
    assert coef32 == min(mn / (0.5 * norm + 1e-6), 1.0) and scale == 0.5 * coef32


@pytest.mark.parametrize("norm_type", [2.0, math.inf], ids=["l2", "max"])
@pytest.mark.parametrize("kind", ["normal", "huge"])
def test_torch_fp32_results_against_the_gpu_tests_bound(norm_type, kind):
    """torch on the input the kernel gets (the flat arena as ONE fp32 tensor), against the restatement with the bound of the
    GPU tests, (2^-24 + n 2^-52) |ref|:
      - the kernel's recipe spelt in torch -- fp32 values, squares added in double, ONE rounding to fp32
        (linalg.vector_norm(dtype=float64).float()) -- lies inside it, for every range and both norms;
      - the max norm of clip_grad_norm_ in fp32 is exact, so it lies inside it too;
      - the L2 norm of clip_grad_norm_ in fp32 does NOT always: torch's CPU kernel squares and adds in fp32 (the huge range
        overflows to inf; on other seeds of the normal range its error was measured at up to 3.4 x this bound).  What holds
        for it a priori is the fp32 sum's own term, n roundings on the sum halved by the root plus the root's: (1 + n / 2) u.
        That is the reason the kernel accumulates in double, and why its bound can be this tight.
    The clipped gradients of clip_grad_norm_ carry three more fp32 roundings (norm + 1e-6, the division, the product)."""
    g = _arena(_tensors(4, torch.float32, kind))
    n = g.numel()
    max_norm = R.f32(0.5 * R.clip_ref(g, math.inf, norm_type)[0])
    norm, coef, _, flag = R.clip_ref(g, max_norm, norm_type)
    assert not flag and coef < 1.0
    recipe = float(torch.linalg.vector_norm(g, norm_type, dtype=torch.float64).float())
    ratio = abs(recipe - norm) / R.relative_bound(norm, n)
    print(f"fp32 values, double sum, one rounding, {kind}/{norm_type}: |norm - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    p = torch.nn.Parameter(torch.zeros_like(g))
    p.grad = g.clone()
    got = float(torch.nn.utils.clip_grad_norm_([p], max_norm, norm_type))
    if kind == "huge" and norm_type == 2.0:
        assert math.isinf(got), "torch's fp32 sum of squares overflows where the double sum does not"
        return
    ratio = abs(got - norm) / R.relative_bound(norm, n)
    print(f"clip_grad_norm_ in fp32, {kind}/{norm_type}: |norm - ref| / bound = {ratio:.3f}")
    if norm_type == math.inf:
        assert ratio <= 1.0
    own = ((1 + n / 2) * R.U32 if norm_type == 2.0 else R.U32) * norm
    assert abs(got - norm) <= own
    want = g.double() * coef
    rel = 3 * R.U32 + 2 * own / norm            # coef inherits the norm's error; three roundings after it
    assert ((p.grad.double() - want).abs() <= rel * want.abs()).all()


def test_restatement_on_the_edge_ranges():
    z = R.clip_ref(torch.zeros(9), 1.0)
    assert z == (0.0, 1.0, 1.0, False)
    h = R.values("huge", 1025, 1)
    assert torch.isinf((h * h).sum()) and torch.isinf(h * h).any()
    norm, coef, scale, flag = R.clip_ref(h, 1.0)
    assert math.isfinite(norm) and not flag and abs(norm - float(h.double().norm())) <= 1e-12 * norm
    t = R.values("tiny", 1025, 1)
    assert not (t * t).any()
    norm, coef, scale, flag = R.clip_ref(t, 1.0)
    assert 0 < norm < R.F32_MIN_NORMAL and coef == 1.0 and abs(norm - float(t.double().norm())) <= 1e-12 * norm
    for nt in (2.0, "inf"):
        norm, coef, scale, flag = R.clip_ref(R.values("nan", 33, 1), 1.0, nt)
        assert math.isnan(norm) and math.isnan(coef) and math.isnan(scale) and flag
        norm, coef, scale, flag = R.clip_ref(R.values("inf", 33, 1), 1.0, nt)
        assert norm == math.inf and coef == 0.0 and scale == 0.0 and flag
        # torch agrees on both (error_if_nonfinite=False): the norm it returns and the coefficient it applies
        for kind in ("nan", "inf"):
            p = torch.nn.Parameter(torch.zeros(33, dtype=torch.float64))
            p.grad = R.values(kind, 33, 1).double()
            got = float(torch.nn.utils.clip_grad_norm_([p], 1.0, float(nt)))
            want = R.clip_ref(R.values(kind, 33, 1), 1.0, nt)
            assert (math.isnan(got) and math.isnan(want[0])) or got == want[0]
            assert bool(torch.isnan(p.grad[0])) == math.isnan(want[1]) and (kind == "nan" or p.grad[0] == 0.0)
    assert R.clip_ref(R.values("normal", 33, 1), math.inf, 2.0, gscale=0.25)[1:3] == (1.0, 0.25)
    # the bound: relative for normal results, half a subnormal spacing below
    assert R.bound(3.0, 1024) == R.relative_bound(3.0, 1024) == (2.0 ** -24 + 1024 * 2.0 ** -52) * 3.0
    assert R.bound(1e-39, 4) == 2.0 ** -150 + 4 * 2.0 ** -52 * 1e-39


# ------------------------------------------------------------------------------------------------ configuration
def _gc(**kw):
    from semivl_amd.optim import grad_clip_from_cfg
    return grad_clip_from_cfg(dict(optimizer_config=dict(grad_clip=dict(**kw))))


def test_grad_clip_from_cfg_accepts():
    from semivl_amd.optim import grad_clip_from_cfg
    from semivl_amd.train import grad_clip_from_cfg as exported
    assert exported is grad_clip_from_cfg
    assert grad_clip_from_cfg({}) is None
    assert grad_clip_from_cfg(dict(optimizer_config=None)) is None
    assert grad_clip_from_cfg(dict(optimizer_config={})) is None
    assert grad_clip_from_cfg(dict(optimizer_config=dict(grad_clip=None))) is None
    assert grad_clip_from_cfg(dict(optimizer_config=dict(type="OptimizerHook", grad_clip=None))) is None
    assert _gc(max_norm=35) == dict(max_norm=35.0, norm_type=2.0)
    assert _gc(max_norm=0.5, norm_type=2) == dict(max_norm=0.5, norm_type=2.0)
    assert _gc(max_norm=1.0, norm_type=2.0) == dict(max_norm=1.0, norm_type=2.0)
    assert _gc(max_norm=1.0, norm_type=float("inf")) == dict(max_norm=1.0, norm_type=math.inf)
    assert _gc(max_norm=1.0, norm_type="inf") == dict(max_norm=1.0, norm_type=math.inf)
    assert _gc(max_norm=float("inf")) == dict(max_norm=math.inf, norm_type=2.0)
    assert _gc(max_norm=1.0, error_if_nonfinite=False, foreach=True) == dict(max_norm=1.0, norm_type=2.0)
    assert _gc(max_norm=1.0, foreach=None) == dict(max_norm=1.0, norm_type=2.0)
    got = grad_clip_from_cfg(dict(optimizer_config=dict(type="OptimizerHook", grad_clip=dict(max_norm=2))))
    assert got == dict(max_norm=2.0, norm_type=2.0) and isinstance(got["max_norm"], float)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("-inf"), True, False, "1.0", None, [1.0]])
def test_grad_clip_from_cfg_refuses_a_bad_max_norm(bad):
    with pytest.raises(ValueError, match="max_norm"):
        _gc(max_norm=bad)


def test_grad_clip_from_cfg_raises():
    from semivl_amd.optim import grad_clip_from_cfg
    with pytest.raises(ValueError, match="max_norm"):
        _gc(norm_type=2)
    with pytest.raises(ValueError, match="clip_value"):
        _gc(max_norm=1.0, clip_value=0.1)
    with pytest.raises(ValueError, match="grad_clip"):
        grad_clip_from_cfg(dict(optimizer_config=dict(grad_clip=35)))
    with pytest.raises(ValueError, match="optimizer_config"):
        grad_clip_from_cfg(dict(optimizer_config=35))
    for nt in (1, 1.0, 3, 0.5, float("-inf"), float("nan"), "2", "fro", True, None):
        with pytest.raises(NotImplementedError, match="norm_type"):
            _gc(max_norm=1.0, norm_type=nt)
    with pytest.raises(NotImplementedError, match="error_if_nonfinite"):
        _gc(max_norm=1.0, error_if_nonfinite=True)
    for key in ("cumulative_iters", "loss_scale", "distributed"):
        with pytest.raises(NotImplementedError, match=key):
            grad_clip_from_cfg(dict(optimizer_config={"grad_clip": dict(max_norm=1.0), key: 2}))
        with pytest.raises(NotImplementedError, match=key):
            grad_clip_from_cfg(dict(optimizer_config={key: 2}))


def test_optimizer_from_cfg_hands_the_clip_to_every_branch(monkeypatch):
    """The dispatch without a GPU: stand-ins record what optimizer_from_cfg / build_optimizer pass on.  Without the key
    (or with grad_clip=None) the constructors are called exactly as before -- no grad_clip argument at all."""
    from semivl_amd import optim as T
    seen = []

    class Adam:
        def __init__(self, model, ocfg, ema_decay=None, **kw):
            seen.append(("AdamW", ema_decay, kw))

    class Sgd:
        def __init__(self, model, ocfg, ema_decay=None, **kw):
            seen.append(("SGD", ema_decay, kw))

        @classmethod
        def original(cls, model, lr, lr_multi, momentum=0.9, weight_decay=1e-4, ema_decay=None, **kw):
            seen.append(("original", ema_decay, kw))

    monkeypatch.setattr(T, "FusedAdamW", Adam)
    monkeypatch.setattr(T, "FusedSGD", Sgd)
    on = dict(grad_clip=dict(max_norm=1.0, norm_type=2.0))
    oc = dict(optimizer_config=dict(grad_clip=dict(max_norm=1.0)))
    T.optimizer_from_cfg(None, dict(lr=0.001, lr_multi=10.0))
    T.optimizer_from_cfg(None, dict(lr=0.001, lr_multi=10.0, **oc))
    T.optimizer_from_cfg(None, dict(optimizer=dict(type="AdamW", lr=0.1), **oc), ema_decay=0.99)
    T.optimizer_from_cfg(None, dict(optimizer=dict(type="SGD", lr=0.1), optimizer_config=dict(
        grad_clip=dict(max_norm=3, norm_type="inf"))))
    T.optimizer_from_cfg(None, dict(optimizer=dict(type="SGD", lr=0.1), optimizer_config=dict(grad_clip=None)))
    T.optimizer_from_cfg(None, dict(optimizer=dict(type="AdamW", lr=0.1), optimizer_config=None))
    T.build_optimizer(None, dict(type="SGD", lr=0.3), grad_clip=dict(max_norm=2.0, norm_type=2.0))
    T.build_optimizer(None, dict(type="AdamW", lr=0.3))
    assert seen == [("original", None, {}), ("original", None, on), ("AdamW", 0.99, on),
                    ("SGD", None, dict(grad_clip=dict(max_norm=3.0, norm_type=math.inf))), ("SGD", None, {}),
                    ("AdamW", None, {}), ("SGD", None, dict(grad_clip=dict(max_norm=2.0, norm_type=2.0))),
                    ("AdamW", None, {})]
    # a bad clip is refused before any optimizer is built
    n = len(seen)
    with pytest.raises(NotImplementedError, match="cumulative_iters"):
        T.optimizer_from_cfg(None, dict(lr=0.001, lr_multi=10.0, optimizer_config=dict(cumulative_iters=2)))
    with pytest.raises(ValueError, match="max_norm"):
        T.optimizer_from_cfg(None, dict(optimizer=dict(lr=0.1), optimizer_config=dict(grad_clip=dict(max_norm=-1))))
    assert len(seen) == n


def test_set_grad_clip_validates_like_the_cfg():
    from semivl_amd.optim import _check_grad_clip
    assert _check_grad_clip(1, "inf") == (1.0, math.inf) and _check_grad_clip(math.inf, 2) == (math.inf, 2.0)
    with pytest.raises(ValueError):
        _check_grad_clip(0.0, 2.0)
    with pytest.raises(NotImplementedError):
        _check_grad_clip(1.0, 1.0)
