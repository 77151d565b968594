"""CPU: the float64 restatement of the mean teacher's arithmetic (tests/ema_ref.py) against independent expressions -- the
arithmetic mean, the closed geometric sum -- the package's schedule against the restated one, a plain fp32 evaluation inside
the a-priori bounds the GPU tests use, and the validation of cfg['ema']."""
import numpy as np
import pytest

import ema_ref as R


def _series(T, n=257, seed=0):
    g = np.random.default_rng(seed)
    start = g.standard_normal(n).astype(np.float32)
    return start, [(g.standard_normal(n) * (1.0 + 0.1 * t)).astype(np.float32) for t in range(T)]


@pytest.mark.parametrize("decay", [0.996, 0.9999, 1.0 - 2.0 ** -20])
def test_warmup_recursion_is_the_arithmetic_mean(decay):
    """While 1 - 1 / t < decay the average is the plain mean of p_1 .. p_t, whatever it started from."""
    T = 40
    assert 1.0 - 1.0 / T < decay
    start, vals = _series(T)
    got = R.recursion(vals, decay, True, start)
    for t in range(1, T + 1):
        mean = np.mean(np.asarray(vals[:t], np.float64), axis=0)
        assert np.abs(got[t - 1] - mean).max() <= 1e-12, t
    assert R.schedule(decay, True, 1) == 0.0 and np.array_equal(got[0], np.asarray(vals[0], np.float64))


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.99, 0.996])
def test_constant_decay_is_the_geometric_sum(decay):
    start, vals = _series(25, seed=1)
    got = R.recursion(vals, decay, False, start)
    for T in (1, 2, 3, 25):
        assert np.abs(got[T - 1] - R.geometric_sum(vals[:T], decay, start)).max() <= 1e-12, T


def _bare_optimizer(decay, warmup):
    from semivl_amd.optim import ArenaOptimizer
    opt = object.__new__(ArenaOptimizer)          # the schedule reads two attributes: no arena, no GPU
    opt.ema_decay, opt.ema_warmup = decay, warmup
    return opt


def test_schedule_matches_the_restatement_exactly():
    from semivl_amd.optim import ema_decay_schedule
    for warmup in (True, False):
        opt = _bare_optimizer(0.996, warmup)
        for t in (1, 2, 3, 250, 251):
            assert opt.ema_decay_at(t) == R.schedule(0.996, warmup, t) == ema_decay_schedule(0.996, warmup, t), (warmup, t)
    opt = _bare_optimizer(0.996, True)
    assert [opt.ema_decay_at(t) for t in (1, 2, 3)] == [0.0, 0.5, 1.0 - 1.0 / 3]
    # the switch from 1 - 1 / t to decay sits between t = 250 and t = 251
    assert opt.ema_decay_at(250) == 1.0 - 1.0 / 250 and abs(opt.ema_decay_at(250) - 0.996) <= 2.0 ** -52
    assert opt.ema_decay_at(249) == 1.0 - 1.0 / 249 < 0.996
    assert opt.ema_decay_at(251) == 0.996 < 1.0 - 1.0 / 251 and opt.ema_decay_at(10 ** 6) == 0.996
    assert _bare_optimizer(0.996, False).ema_decay_at(1) == 0.996
    with pytest.raises(ValueError):
        opt.ema_decay_at(0)


@pytest.mark.parametrize("d", [0.0, 0.5, 2.0 / 3, 0.996, 1.0 - 2.0 ** -20])
def test_plain_fp32_evaluation_stays_inside_the_step_bound(d):
    """numpy's fp32 evaluation of the expression as written (three roundings, no FMA) on the GPU tests' kind of data."""
    start, vals = _series(1, n=4099, seed=2)
    d32, omd32 = (np.float32(v) for v in R.kernel_factors(d))
    got = d32 * start + omd32 * vals[0]
    assert got.dtype == np.float32
    ref, bound = R.step_ref(start, vals[0], d)
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    if d == 0.0:
        assert np.array_equal(got, vals[0])


def test_fp32_chain_stays_inside_the_compounded_bound():
    """Three warm-up steps in fp32 against the exact mean: the bound the GPU step test uses."""
    start, vals = _series(3, n=4099, seed=3)
    e = start.copy()
    for t, v in enumerate(vals, 1):
        d32, omd32 = (np.float32(x) for x in R.kernel_factors(R.schedule(0.996, True, t)))
        e = d32 * e + omd32 * v
    mean = np.mean(np.asarray(vals, np.float64), axis=0)
    B = R.compounded_bound(vals, 0.996, True, start)
    assert (np.abs(e.astype(np.float64) - mean) <= B).all() and B.max() < 1e-5


def test_ema_from_cfg_defaults_and_refusals():
    from semivl_amd.optim import ema_from_cfg
    assert ema_from_cfg({}) is None and ema_from_cfg(dict(optimizer=dict(type="AdamW"))) is None
    assert ema_from_cfg(dict(ema=dict(decay=0.996))) == dict(decay=0.996, warmup=True, teacher=True, buffers="ema")
    assert ema_from_cfg(dict(ema=dict(decay=0, warmup=False, teacher=False, buffers="copy"))) == \
        dict(decay=0.0, warmup=False, teacher=False, buffers="copy")
    bad = [(None, "dict"), (0.996, "dict"), ([0.996], "dict"),                       # not a dict
           (dict(), "decay"), (dict(warmup=True), "decay"),                           # decay is required
           (dict(decay=0.9, momentum=0.9), "momentum"),                               # an unknown key
           (dict(decay=True), "decay"), (dict(decay="0.9"), "decay"), (dict(decay=None), "decay"),
           (dict(decay=1.0), "decay"), (dict(decay=-0.1), "decay"), (dict(decay=float("nan")), "decay"),
           (dict(decay=0.9, warmup=1), "warmup"), (dict(decay=0.9, warmup=None), "warmup"),
           (dict(decay=0.9, teacher="yes"), "teacher"), (dict(decay=0.9, teacher=0), "teacher"),
           (dict(decay=0.9, buffers="mean"), "buffers"), (dict(decay=0.9, buffers=None), "buffers")]
    for value, word in bad:
        with pytest.raises(ValueError, match=word):
            ema_from_cfg(dict(ema=value))


def test_optimizer_from_cfg_refuses_two_sources_before_it_touches_the_model():
    from semivl_amd.optim import optimizer_from_cfg

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the model was touched: " + name)

    cfg = dict(optimizer=dict(type="AdamW", lr=1e-3), ema=dict(decay=0.99))
    with pytest.raises(ValueError, match="ema_decay"):
        optimizer_from_cfg(Untouchable(), cfg, ema_decay=0.99)
    with pytest.raises(ValueError, match="buffers"):
        optimizer_from_cfg(Untouchable(), dict(cfg, ema=dict(decay=0.99, buffers="x")))
    with pytest.raises(ValueError, match="decay"):
        optimizer_from_cfg(Untouchable(), dict(lr=1e-3, lr_multi=10.0, ema=dict(decay=1.0)))
