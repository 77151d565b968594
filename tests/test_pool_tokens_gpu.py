"""GPU: the four kernels of csrc/pool_tokens.hip through semivl_amd.ops against the float64 restatements of
tests/pool_tokens_ref.py under the bounds derived there -- no tolerance is chosen here.

Every case runs in two layouts: rows wider than C with a 16-byte aligned channel offset (the 16-byte paths where
C % 4 == 0) and an odd offset in an odd row stride (the scalar paths).  Sources are column slices of sentinel matrices,
destinations are written into sentinel guard bands and gap columns that must come back intact, and every launch runs twice
for a bit-for-bit comparison.  One case per kernel family exceeds a single pass of its capped grid.  -s prints
error / bound."""
import pytest
import torch

import pool_tokens_ref as P

pytestmark = pytest.mark.gpu

ALL = [(c, lay) for c in P.CASES for lay in P.LAYOUTS]
IDS = [f"{c[0]}x{c[1]}x{c[2]}-{lay[0]}" for c, lay in ALL]


def _ratio(tag, got, want, bound):
    err = (got.double() - want).abs()
    z = bound <= 0
    assert bool((err[z] == 0).all()), tag
    r = float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0
    print(f"[{tag}] max error / bound = {r:.3f} over {got.numel()} elements")
    assert r <= 1.0, (tag, r)


def _src(t2d, slack, off, dev):
    rows, C = t2d.shape
    _, v = P.strided(rows, C, C + slack, off, dev, fill=-P.SENTINEL)
    v.copy_(t2d)
    return v


def _twice(tag, rows, C, slack, off, dev, run, init=None):
    """run(view) on two fresh sentinel matrices: bit-identical buffers, gaps and guard bands intact; returns the view."""
    out = []
    for _ in range(2):
        buf, v = P.strided(rows, C, C + slack, off, dev)
        if init is not None:
            v.copy_(init)
        run(v)
        out.append((buf, v))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]), f"{tag}: two runs differ"
    assert P.gaps_intact(out[0][0], rows, C, C + slack, off), f"{tag}: wrote outside its destination"
    return out[0][1]


@pytest.mark.parametrize("case,lay", ALL + [(P.BIG_SUM, P.LAYOUTS[0])], ids=IDS + ["sum_two_passes"])
def test_gap_tokens_fwd(dev, case, lay):
    from semivl_amd import ops
    imgs, HW, C = case
    _, slack, off = lay
    x = P.inputs(case)[0].to(dev)
    xs = _src(x, slack, off, dev)
    want, bound = P.gap_fwd_ref(x, imgs, HW)
    got = _twice("gap_fwd", imgs, C, slack, off, dev, lambda v: ops.gap_tokens_fwd(xs, imgs, HW, out=v))
    _ratio(f"gap_tokens_fwd {case} {lay[0]}", got, want, bound)
    if HW == 1:
        assert torch.equal(got, x)
    # the contiguous call form the head uses (fresh output)
    assert torch.equal(ops.gap_tokens_fwd(xs, imgs, HW), got)


@pytest.mark.parametrize("case,lay", ALL + [(P.BIG_ELTWISE, P.LAYOUTS[0])], ids=IDS + ["eltwise_two_passes"])
def test_gap_tokens_bwd(dev, case, lay):
    from semivl_amd import ops
    imgs, HW, C = case
    _, slack, off = lay
    _, dpool, base = [t.to(dev) for t in P.inputs(case)]
    dps = _src(dpool, slack, off, dev)
    rows = imgs * HW
    want, bound = P.gap_bwd_ref(dpool, imgs, HW)
    plain = _twice("gap_bwd", rows, C, slack, off, dev, lambda v: ops.gap_tokens_bwd(dps, imgs, HW, dx=v))
    _ratio(f"gap_tokens_bwd {case} {lay[0]}", plain, want, bound)
    zero = _twice("gap_bwd +0", rows, C, slack, off, dev, lambda v: ops.gap_tokens_bwd(dps, imgs, HW, dx=v, accumulate=True),
                  init=torch.zeros(rows, C, device=dev))
    assert torch.equal(zero, plain), "accumulate onto zeros"
    acc = _twice("gap_bwd +base", rows, C, slack, off, dev, lambda v: ops.gap_tokens_bwd(dps, imgs, HW, dx=v, accumulate=True),
                 init=base)
    wa, ba = P.gap_bwd_ref(dpool, imgs, HW, base=base)
    _ratio(f"gap_tokens_bwd accumulate {case} {lay[0]}", acc, wa, ba)
    assert torch.equal(ops.gap_tokens_bwd(dps, imgs, HW), plain)


@pytest.mark.parametrize("case,lay", ALL + [(P.BIG_ELTWISE, P.LAYOUTS[0])], ids=IDS + ["eltwise_two_passes"])
def test_bcast_rows_fwd(dev, case, lay):
    """The concat form: the destination is a channel slice [off, off + C) of rows C + slack wide, passed as the whole slab
    plus the channel offset."""
    from semivl_amd import ops
    imgs, HW, C = case
    _, slack, off = lay
    v = P.inputs(case)[1].to(dev)
    vs = _src(v, slack, off, dev)
    rows, ld = imgs * HW, C + slack
    out = []
    for _ in range(2):
        buf, _view = P.strided(rows, C, ld, off, dev)
        slab = buf[P.AGUARD:P.AGUARD + rows * ld].view(rows, ld)
        ops.bcast_rows_fwd(vs, imgs, HW, slab, off)
        out.append((buf, _view))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0])
    assert P.gaps_intact(out[0][0], rows, C, ld, off), "wrote outside its channel slice"
    assert torch.equal(out[0][1], P.bcast_fwd_ref(v, imgs, HW))


@pytest.mark.parametrize("case,lay", ALL + [(P.BIG_SUM, P.LAYOUTS[0])], ids=IDS + ["sum_two_passes"])
def test_bcast_rows_bwd(dev, case, lay):
    from semivl_amd import ops
    imgs, HW, C = case
    _, slack, off = lay
    dy = P.inputs(case)[0].to(dev)
    rows, ld = imgs * HW, C + slack
    buf, view = P.strided(rows, C, ld, off, dev, fill=-P.SENTINEL)
    view.copy_(dy)
    slab = buf[P.AGUARD:P.AGUARD + rows * ld].view(rows, ld)
    want, bound = P.bcast_bwd_ref(dy, imgs, HW)
    got = _twice("bcast_bwd", imgs, C, slack, off, dev, lambda v: ops.bcast_rows_bwd(slab, off, C, imgs, HW, out=v))
    _ratio(f"bcast_rows_bwd {case} {lay[0]}", got, want, bound)
    if HW == 1:
        assert torch.equal(got, dy)
