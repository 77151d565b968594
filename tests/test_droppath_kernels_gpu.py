"""svl_droppath_fwd_f32 / svl_droppath_bwd_f32 on the GPU against their float64 restatement (tests/droppath_ref.py).  Every
output sits between sentinel guard bands, every case runs twice and must agree bit for bit.

Forward: out = resid + s_b * branch with s_b the fp32 product mask[b] * float32(1 / keep): one rounding for the product, one
for the sum (one in all if the compiler contracted the two into an FMA; csrc/droppath.hip asks for __fmul_rn / __fadd_rn), so
per element |err| <= gamma(2) * (|resid| + |s_b * branch|), plus the restatement's own 2^-52 of the same magnitude.  Rows of a
dropped sample are resid's bits.  Backward: one fp32 product, so the result EQUALS the fp32 product s_b * dout; dropped rows are
zeros.  Neither kernel reads the branch / dout rows of a dropped sample: they hold NaN here.  With -s each forward case prints
its worst error / bound ratio.

Shapes: B in {1, 3} x T in {1, 5, 70} x E in {4, 6, 64, 768} (E = 6: the scalar path); three of them again on pointers 4 bytes
off a 16-byte boundary (the alignment fallback); (5, 7, 64) with alternating masks -- 16 rows per workgroup of 256 items, so
every workgroup straddles samples with different scales, as do the (3, 5, *) ones; and two whose item count exceeds one pass
of the capped grid (2048 blocks of 256 threads: 524 288 items, of 4 floats on the 16-byte path, of 1 on the scalar path).  The
forward runs into a third buffer and in place in the branch's buffer."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import droppath_ref as R
from small_kernel_ref import SENTINEL

pytestmark = pytest.mark.gpu

ONE_PASS = 2048 * 256
KEEP = 0.75
# (B, T, E, element offset of every matrix pointer from a 16-byte boundary)
SHAPES = [(B, T, E, 0) for B, T, E in itertools.product((1, 3), (1, 5, 70), (4, 6, 64, 768))]
SHAPES += [(1, 1, 4, 1), (3, 5, 64, 1), (3, 70, 768, 1), (5, 7, 64, 0), (3, 1000, 768, 0), (3, 29200, 6, 0)]
IDS = ["x".join(str(v) for v in s[:3]) + ("-off4" if s[3] else "") for s in SHAPES]
assert 3 * 1000 * 768 // 4 > ONE_PASS and 3 * 29200 * 6 > ONE_PASS
MASKS = ["zeros", "ones", "mixed"]


def _mask(kind, B):
    if kind == "mixed":
        return torch.tensor([float(1 - b % 2) for b in range(B)]) if B > 1 else torch.tensor([1.0])
    return torch.zeros(B) if kind == "zeros" else torch.ones(B)


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


def _inputs(B, T, E, mask, seed):
    """branch / resid / dout [B * T, E]; the branch and dout rows of dropped samples are NaN (the kernels must not read them)"""
    g = torch.Generator().manual_seed(seed)
    branch, resid, dout = (torch.randn(B * T, E, generator=g) for _ in range(3))
    drop = (mask == 0).repeat_interleave(T)
    branch[drop] = float("nan")
    dout[drop] = float("nan")
    return branch, resid, dout, drop.numpy()


@pytest.mark.parametrize("alias", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fwd_matches_fp64_within_two_roundings(dev, shape, kind, alias):
    from semivl_amd import ops
    B, T, E, off = shape
    mask = _mask(kind, B)
    branch, resid, _, drop = _inputs(B, T, E, mask, seed=B * T + E)
    n = B * T * E
    s = R.sample_scale(mask.numpy(), R.scale32(KEEP))
    ref, mag = R.droppath_fwd_ref(branch.numpy(), resid.numpy(), s, T)
    _, rd = _buf(n, off, dev, resid)
    _, md = _buf(B, 0, dev, mask)
    bufs = []
    for _ in range(2):
        bb, bp = _buf(n, off, dev, branch)
        if alias:
            out = ops.droppath_add(bp.view(B * T, E), rd.view(B * T, E), md, KEEP, B, T)
            assert out.data_ptr() == bp.data_ptr()
            bufs.append(bb)
        else:
            ob, op = _buf(n, off, dev)
            ops.droppath_add(bp.view(B * T, E), rd.view(B * T, E), md, KEEP, B, T, out=op.view(B * T, E))
            assert _intact(bb, n, off) and np.array_equal(bp.cpu().numpy(), branch.reshape(-1).numpy(), equal_nan=True)   # only read
            bufs.append(ob)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1]) and _intact(bufs[0], n, off)
    assert torch.equal(rd.cpu(), resid.reshape(-1))                 # resid is only read
    got = bufs[0][64 + off:64 + off + n].view(B * T, E).cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got[drop], resid.numpy()[drop])           # rows of dropped samples: resid's bits
    err = np.abs(got.astype(np.float64) - ref)
    bound = (R.gamma(2) + 2.0 ** -52) * mag
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"droppath_fwd B={B} T={T} E={E} off={off} mask={kind} {'in place' if alias else 'out'}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bwd_equals_the_fp32_product(dev, shape, kind):
    from semivl_amd import lib as L, ops
    B, T, E, off = shape
    mask = _mask(kind, B)
    _, _, dout, drop = _inputs(B, T, E, mask, seed=B * T + E + 1)
    n = B * T * E
    s32 = (mask.numpy() * np.float32(R.scale32(KEEP))).astype(np.float32)
    keepr = ~drop
    want = np.zeros((B * T, E), dtype=np.float32)
    want[keepr] = np.repeat(s32, T)[keepr, None] * dout.numpy()[keepr]      # fp32 numpy: one rounding
    assert want.dtype == np.float32
    ref = R.droppath_bwd_ref(dout.numpy(), R.sample_scale(mask.numpy(), R.scale32(KEEP)), T)
    assert np.array_equal(want, ref.astype(np.float32))             # and so the fp32 rounding of the float64 restatement
    _, dd = _buf(n, off, dev, dout)
    _, md = _buf(B, 0, dev, mask)
    # the wrapper allocates its own (aligned) result; the raw entry point writes between guard bands at the case's offset
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bufs = []
    for _ in range(2):
        ob, op = _buf(n, off, dev)
        L.check(L.load().svl_droppath_bwd_f32(C.c_void_p(dd.data_ptr()), C.c_void_p(md.data_ptr()), R.scale32(KEEP),
                                              C.c_void_p(op.data_ptr()), B, T, E, st), "svl_droppath_bwd_f32")
        bufs.append(ob)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1]) and _intact(bufs[0], n, off)
    got = bufs[0][64 + off:64 + off + n].view(B * T, E).cpu().numpy()
    assert np.array_equal(got, want) and not got[drop].any()
    if off == 0:
        w = ops.droppath_scale(dd.view(B * T, E), md, KEEP, B, T)
        assert w.data_ptr() != dd.data_ptr() and np.array_equal(w.cpu().numpy(), want)
    assert np.array_equal(dd.cpu().numpy(), dout.reshape(-1).numpy(), equal_nan=True)    # dout is only read


def test_workgroups_that_straddle_samples_use_both_scales(dev):
    """(5, 7, 64) with masks 1 0 1 0 1 and different values per sample position: every row of the result is its own sample's --
    a kernel that took one scale per workgroup (16 rows here) or per wave (4 rows) would fail rows 7.., 14.., 21.., 28.."""
    from semivl_amd import ops
    B, T, E = 5, 7, 64
    mask = _mask("mixed", B).to(dev)
    branch = torch.ones(B * T, E, device=dev)
    resid = torch.zeros(B * T, E, device=dev)
    out = ops.droppath_add(branch.clone(), resid, mask, 0.5, B, T)
    db = ops.droppath_scale(branch, mask, 0.5, B, T)
    want = (mask * 2.0).repeat_interleave(T)[:, None].expand(B * T, E)
    assert torch.equal(out, want) and torch.equal(db, want)


def test_bad_arguments_are_refused_and_write_nothing(dev):
    import semivl_amd.lib as L
    lib = L.load()
    B, T, E = 2, 4, 8
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bo, po = _buf(B * T * E, 0, dev)
    src = torch.randn(B * T * E, device=dev)
    mask = torch.ones(B, device=dev)
    for args in ((p(src), p(src), p(mask), 1.0, p(po), 0, T, E), (p(src), p(src), p(mask), 1.0, p(po), B, 0, E),
                 (p(src), p(src), p(mask), 1.0, p(po), B, T, -1), (None, p(src), p(mask), 1.0, p(po), B, T, E),
                 (p(src), None, p(mask), 1.0, p(po), B, T, E), (p(src), p(src), None, 1.0, p(po), B, T, E),
                 (p(src), p(src), p(mask), 1.0, None, B, T, E), (p(src), p(po), p(mask), 1.0, p(po), B, T, E)):
        assert lib.svl_droppath_fwd_f32(*args, st) < 0 and "svl_droppath_fwd_f32" in L.last_error()
    for args in ((p(src), p(mask), 1.0, p(po), 0, T, E), (p(src), p(mask), 1.0, p(po), B, -3, E),
                 (p(src), p(mask), 1.0, p(po), B, T, 0), (None, p(mask), 1.0, p(po), B, T, E),
                 (p(src), None, 1.0, p(po), B, T, E), (p(src), p(mask), 1.0, None, B, T, E)):
        assert lib.svl_droppath_bwd_f32(*args, st) < 0 and "svl_droppath_bwd_f32" in L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(bo, torch.full_like(bo, SENTINEL))
