"""svl_ema_segments_f32 on the GPU against its float64 restatement (tests/ema_ref.py, proven on the CPU by
tests/test_ema_ref.py).  No tolerance is picked: per element |out - ref| <= gamma(n) (|d32 dst| + |omd32 src|) with
n = ema_ref.N_ROUNDINGS_SEGMENTS = 2, the fp32 roundings on the kernel's chain as written (csrc/ema.hip:
__fmaf_rn(decay, d, __fmul_rn(omd, s)) -- one rounded product and one fused multiply-add; the intrinsics leave the compiler
no contraction to choose, so there is nothing further to allow for), d32 / omd32 the two fp32 factors the kernel multiplies
with.  Every segment lies between sentinel guard bands; the worst error / bound ratio of every case is
printed (-s)."""
import pytest
import torch

import ema_ref as R
from small_kernel_ref import SENTINEL

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 4, 5, 64, 255, 256, 257, 1025]
GRID_CAP = 256                                   # csrc/ema.hip: EMA_GRID_CAP blocks, one segment per block and trip
NSEGS = [1, 2, 40, 2 * GRID_CAP + 3]             # the last one: every block takes a third trip
DECAYS = [0.0, 0.5, 0.996, 1.0 - 2.0 ** -20]
GUARD = 8                                        # floats, a multiple of 4: the alignment of a payload is its shift alone


def _lengths(nseg):
    return [LENGTHS[(3 * i + nseg) % len(LENGTHS)] for i in range(nseg)]


def _place(lengths, shift, dev, values):
    """(buffer, [payload views], [payload offsets]): every segment between GUARD sentinel floats on each side, its first
    element `shift` floats (4 * shift bytes) past a 16-byte boundary.  values: one CPU tensor per segment."""
    offs, o = [], 0
    for n in lengths:
        o += GUARD
        offs.append(o + shift)
        o += (n + shift + 3) // 4 * 4
    o += GUARD
    buf = torch.full((o,), SENTINEL, device=dev)
    assert buf.data_ptr() % 16 == 0
    views = []
    for off, n, v in zip(offs, lengths, values):
        buf[off:off + n] = v.to(dev)
        views.append(buf[off:off + n])
        assert views[-1].data_ptr() % 16 == 4 * shift
    return buf, views, offs


def _guards_intact(buf, lengths, offs):
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    for off, n in zip(offs, lengths):
        keep[off:off + n] = False
    return bool((buf[keep] == SENTINEL).all())


def _data(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    dst = [torch.randn(n, generator=g) * 3.0 for n in lengths]
    src = [torch.randn(n, generator=g) + 0.5 for n in lengths]
    return dst, src


def _run(dev, lengths, dst0, src0, decay, dshift=0, sshift=0):
    """One guarded call; returns the flat result (CPU).  Checks the guard bands of dst and that src is untouched."""
    from semivl_amd import ops
    dbuf, dviews, doffs = _place(lengths, dshift, dev, dst0)
    sbuf, sviews, soffs = _place(lengths, sshift, dev, src0)
    skeep = sbuf.clone()
    tabs = ops.ema_segment_tables(dviews, sviews)
    assert tabs[3] == len(lengths) and tabs[2].tolist()[-1] == sum(lengths)
    ops.ema_segments(*tabs, decay)
    torch.cuda.synchronize()
    assert _guards_intact(dbuf, lengths, doffs), "guard bands of dst written"
    assert torch.equal(sbuf, skeep), "src written"
    return torch.cat([v.cpu() for v in dviews])


def _ratio(got, dst0, src0, decay):
    ref, bound = R.step_ref(torch.cat(dst0).double().numpy(), torch.cat(src0).double().numpy(), decay,
                            n=R.N_ROUNDINGS_SEGMENTS)
    err = abs(got.double().numpy() - ref)
    live = bound > 0
    assert not err[~live].any()
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("nseg", NSEGS)
def test_segments_within_bound(dev, nseg, decay):
    """Every segment length (nseg = 1: each length on its own), aligned and with dst, src or both 4 bytes off a 16-byte
    boundary (the scalar path: the same bits), twice (bit for bit); decay = 0 reproduces src's bits."""
    worst = 0.0
    for k, lengths in enumerate([[n] for n in LENGTHS] if nseg == 1 else [_lengths(nseg)]):
        dst0, src0 = _data(lengths, seed=100 * nseg + k)
        a = _run(dev, lengths, dst0, src0, decay)
        assert _same(a, _run(dev, lengths, dst0, src0, decay)), "two runs differ"
        for dshift, sshift in ((1, 0), (0, 1), (1, 1)):
            assert _same(a, _run(dev, lengths, dst0, src0, decay, dshift, sshift)), \
                f"the scalar path (dst + {4 * dshift} B, src + {4 * sshift} B) does not reproduce the 16-byte path"
        if decay == 0.0:
            assert _same(a, torch.cat(src0)), "decay = 0 must reproduce src"
        else:
            assert not _same(a, torch.cat(src0)) and not _same(a, torch.cat(dst0))
        worst = max(worst, _ratio(a, dst0, src0, decay))
    print(f"svl_ema_segments_f32 nseg {nseg}, decay {decay!r}: worst error / bound = {worst:.3f} (n = {R.N_ROUNDINGS_SEGMENTS})")
    assert worst <= 1.0


def test_refusals_and_the_empty_table(dev):
    from semivl_amd import lib as L
    from semivl_amd import ops
    lib = L.load()
    a, b = torch.ones(8, device=dev), torch.full((8,), 3.0, device=dev)
    with pytest.raises(ValueError, match="svl_ema_segments_f32: dst == src"):
        ops.ema_segment_tables([b, a], [a, a])
    with pytest.raises(ValueError, match="svl_ema_segments_f32"):
        ops.ema_segment_tables([a[:6]], [a[2:]])                 # a written segment overlaps what another one reads
    dt, st, off, n = ops.ema_segment_tables([a], [b])

    def status(d=dt, s=st, o=off, nseg=n, decay=0.5):
        return lib.svl_ema_segments_f32(ops._p(d), ops._p(s), ops._p(o), nseg, decay, ops._st())

    for kw in (dict(s=dt), dict(d=None), dict(s=None), dict(o=None), dict(nseg=-1), dict(decay=-0.5), dict(decay=1.5),
               dict(decay=float("nan"))):
        assert status(**kw) == -1 and "svl_ema_segments_f32" in L.last_error(), kw
    assert status(s=dt) == -1 and "dst == src" in L.last_error()
    assert status(d=None, s=None, o=None, nseg=0) == 0           # nothing to do: no launch, nothing read
    torch.cuda.synchronize()
    assert bool((a == 1.0).all()) and bool((b == 3.0).all()), "a refused call wrote"
    empty = ops.ema_segment_tables([], [])
    ops.ema_segments(*empty, 0.5)
    assert status() == 0
    torch.cuda.synchronize()
    assert bool((a == 2.0).all()) and bool((b == 3.0).all())
