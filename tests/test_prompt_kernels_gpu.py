"""svl_prompt_rows_fwd_f32 / svl_prompt_rows_bwd_f32 on the GPU against their float64 restatement (tests/prompt_ref.py).  Every
output sits between sentinel guard bands, every case runs twice and must agree bit for bit.

Forward: nothing is summed, so the results are BIT-EQUAL to fp32 arithmetic: a prompt row is emb * (mask * float32(scale)) with
each product rounded once (the mask is 0 / 1, so the inner product is exact and the row is the fp32 rounding of the float64
restatement), every other row is a copy; the in-place form leaves every non-prompt row untouched.

Backward: demb[j, e] is one chain per element (csrc/prompt_tokens.hip, every operation an explicit __fmul_rn / __fadd_rn):
the term dx * (mask * scale) takes 2 roundings (the inner product counted although it is exact for a 0 / 1 mask), none without
a mask; the terms are added in ascending b onto 0 (the first addition is exact), B - 1 roundings; an accumulating call adds
the previous value, 1 more.  So the bound is, per element, gamma(n) times the sum of the absolute terms with

    n = B + 1 + accumulate   with a mask,        n = B - 1 + accumulate   without

(n = 0: the result is exact), plus the float64 restatement's own B * 2^-53.  The zeroed / compacted matrices are bit-equal.
With -s each case prints its worst error / bound ratio.

Shapes (B, T, P, E): (1, 2, 1, 6), (3, 4, 5, 64), (2, 65, 3, 768) and -- on pointers 4 bytes off a 16-byte boundary, so the
scalar path is reached through E % 4 and through the alignment -- (2, 9, 10, 770); the 16-byte
path's shapes again on such pointers (the alignment fallback), and two whose item count exceeds one pass of the capped grid
(256 * 32 blocks of 256 threads: 2 097 152 items, of 4 floats on the 16-byte path, of 1 on the scalar path)."""
import ctypes as C

import numpy as np
import pytest
import torch

import prompt_ref as R
from small_kernel_ref import SENTINEL

pytestmark = pytest.mark.gpu

ONE_PASS = 256 * 32 * 256
# (B, T, P, E, element offset of every pointer from a 16-byte boundary)
SHAPES = [(1, 2, 1, 6, 0), (3, 4, 5, 64, 0), (2, 65, 3, 768, 0), (2, 9, 10, 770, 1), (3, 4, 5, 64, 1), (2, 65, 3, 768, 1),
          (6, 1850, 10, 768, 0), (3, 1000, 3, 771, 0)]
IDS = ["1x2x1x6", "3x4x5x64", "2x65x3x768", "2x9x10x770-off4", "3x4x5x64-off4", "2x65x3x768-off4", "two-passes-vec",
       "two-passes-scalar"]
assert 6 * 1850 * 768 // 4 > ONE_PASS and 3 * 1000 * 771 > ONE_PASS


def _buf(n, off, dev, fill=None):
    """(buffer, payload of n floats `off` elements past a 16-byte boundary) between 64 + off and 64 - off sentinel elements"""
    buf = torch.full((n + 128,), SENTINEL, device=dev)
    pay = buf[64 + off:64 + off + n]
    assert pay.data_ptr() % 16 == 4 * off
    if fill is not None:
        pay.copy_(fill.reshape(-1))
    return buf, pay


def _intact(buf, n, off):
    s = torch.full((1,), SENTINEL, device=buf.device)
    return bool((buf[:64 + off] == s).all()) and bool((buf[64 + off + n:] == s).all())


def _inputs(B, T, P, E, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(B, T, E, generator=g)
    emb = torch.randn(P, E, generator=g)
    mask = (torch.rand(B, P, E, generator=g) < 0.9).float()
    dx = torch.randn(B, T + P, E, generator=g)
    base = torch.randn(P, E, generator=g)
    return src, emb, mask, dx, base


@pytest.mark.parametrize("form", ["expand", "inplace"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fwd_is_bit_equal_to_fp32_arithmetic(dev, shape, masked, form):
    from semivl_amd import ops
    B, T, P, E, off = shape
    src, emb, mask, _, _ = _inputs(B, T, P, E, seed=B * T + P)
    n = B * (T + P) * E
    rows = emb.numpy()[None].repeat(B, 0)
    if masked:
        rows = rows * (mask.numpy() * np.float32(R.SCALE))       # fp32 numpy: each product rounded once
    assert rows.dtype == np.float32
    old = torch.randn(B, T + P, E, generator=torch.Generator().manual_seed(3))       # what the in-place form finds
    ref = R.rows_fwd_ref(emb.numpy(), mask.numpy() if masked else None, R.SCALE,
                         **(dict(src=src.numpy()) if form == "expand" else dict(dst=old.numpy())))
    _, sd = _buf(B * T * E, off, dev, src)
    _, ed = _buf(P * E, off, dev, emb)
    _, md = _buf(B * P * E, off, dev, mask)
    bufs = []
    for _ in range(2):
        buf, pay = _buf(n, off, dev, None if form == "expand" else old)
        ops.prompt_rows_fwd(ed.view(P, E), B, P, pay.view(B * (T + P), E), src=sd.view(B * T, E) if form == "expand" else None,
                            mask=md.view(B, P, E) if masked else None, scale=1.0 / 0.9)
        bufs.append(buf)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1]) and _intact(bufs[0], n, off)
    got = bufs[0][64 + off:64 + off + n].view(B, T + P, E).cpu().numpy()
    assert np.array_equal(got[:, 1:1 + P], rows)
    other = src.numpy() if form == "expand" else np.delete(old.numpy(), np.s_[1:1 + P], axis=1)
    assert np.array_equal(got[:, 0], other[:, 0]) and np.array_equal(got[:, 1 + P:], other[:, 1:])
    assert np.array_equal(got, ref.astype(np.float32))           # and so the fp32 rounding of the float64 restatement


@pytest.mark.parametrize("form", ["zero", "compact"])
@pytest.mark.parametrize("acc", [False, True], ids=["write", "acc"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bwd_matches_fp64_within_the_rounding_bound(dev, shape, masked, acc, form):
    from semivl_amd import ops
    B, T, P, E, off = shape
    _, _, mask, dx, base = _inputs(B, T, P, E, seed=B * T + P + 1)
    demb, mag, zeroed, compact = R.rows_bwd_ref(dx.numpy(), P, mask.numpy() if masked else None, R.SCALE,
                                                demb0=base.numpy() if acc else None)
    n, nc = B * (T + P) * E, B * T * E
    _, md = _buf(B * P * E, off, dev, mask)
    runs = []
    for _ in range(2):
        bx, px = _buf(n, off, dev, dx)
        be, pe = _buf(P * E, off, dev, base if acc else None)
        bc, pc = _buf(nc, off, dev) if form == "compact" else (None, None)
        ops.prompt_rows_bwd(px.view(B * (T + P), E), B, P, out=pe.view(P, E), mask=md.view(B, P, E) if masked else None,
                            scale=1.0 / 0.9, accumulate=acc, compact=pc.view(B * T, E) if form == "compact" else None)
        runs.append((bx, be, bc))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert a is None or torch.equal(a, b)
    bx, be, bc = runs[0]
    assert _intact(bx, n, off) and _intact(be, P * E, off) and (bc is None or _intact(bc, nc, off))
    gx = bx[64 + off:64 + off + n].view(B, T + P, E).cpu().numpy()
    if form == "zero":
        assert np.array_equal(gx, zeroed.astype(np.float32))
    else:
        assert np.array_equal(gx, dx.numpy())                   # the compact form only reads dx
        assert np.array_equal(bc[64 + off:64 + off + nc].view(B, T, E).cpu().numpy(), compact.astype(np.float32))
    nr = (B + 1 if masked else B - 1) + (1 if acc else 0)
    err = np.abs(be[64 + off:64 + off + P * E].view(P, E).double().cpu().numpy() - demb)
    bound = (R.gamma(nr) + B * 2.0 ** -53) * mag
    assert np.isfinite(err).all()
    if nr == 0:
        assert not err.any()
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"prompt_rows_bwd B={B} T={T} P={P} E={E} off={off} mask={masked} accumulate={acc} {form}: n = {nr}, "
          f"worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_bwd_without_a_sum_only_zeroes(dev):
    """out=None (every prompt tensor frozen): the rows are zeroed, nothing else happens"""
    from semivl_amd import ops
    B, T, P, E = 2, 5, 3, 64
    dx = torch.randn(B, T + P, E, generator=torch.Generator().manual_seed(9))
    bx, px = _buf(dx.numel(), 0, dev, dx)
    ops.prompt_rows_bwd(px.view(B * (T + P), E), B, P)
    torch.cuda.synchronize()
    want = dx.clone()
    want[:, 1:1 + P] = 0
    assert torch.equal(px.view(B, T + P, E).cpu(), want) and _intact(bx, dx.numel(), 0)


def test_bad_arguments_are_refused_and_write_nothing(dev):
    import semivl_amd.lib as L
    lib = L.load()
    B, T, P, E = 2, 4, 3, 8
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bd, pd = _buf(B * (T + P) * E, 0, dev)
    be, pe = _buf(P * E, 0, dev)
    src = torch.randn(B * T * E, device=dev)
    for args in ((p(src), None, p(pe), None, 1.0, B, T, P, E), (p(src), p(pd), None, None, 1.0, B, T, P, E),
                 (p(src), p(pd), p(pe), None, 1.0, B, T, 0, E), (p(src), p(pd), p(pe), None, 1.0, 0, T, P, E),
                 (p(pd), p(pd), p(pe), None, 1.0, B, T, P, E)):
        assert lib.svl_prompt_rows_fwd_f32(*args, st) < 0 and "svl_prompt_rows_fwd_f32" in L.last_error()
    for args in ((None, None, p(pe), None, 1.0, 0, B, T, P, E), (p(pd), None, p(pe), None, 1.0, 0, B, T, P, 0),
                 (p(pd), p(pd), p(pe), None, 1.0, 0, B, T, P, E)):
        assert lib.svl_prompt_rows_bwd_f32(*args, st) < 0 and "svl_prompt_rows_bwd_f32" in L.last_error()
    torch.cuda.synchronize()
    for buf in (bd, be):
        assert torch.equal(buf, torch.full_like(buf, SENTINEL))
