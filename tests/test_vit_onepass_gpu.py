"""GPU: the one-pass forms of the ViT glue between GEMMs, bit for bit against the sequences they replace (which stay in the
library): svl_layernorm_{fwd,bwd}_pack_f16x2 against the row kernel followed by svl_split_planes_f16x2 (planes-only forward:
against svl_layernorm_fwd_planes_f16x2), the tensor_amax by-product of the pack passes against the exact maximum an
operand-maximum pass finds, and svl_gemm_f32 with supplied maxima against the same call with its own maximum passes.

Every comparison is torch.equal on int32 views (NaN-proof, sign-of-zero-proof).  Buffers a kernel may leave partly unwritten
(plane padding, sexp / rnorm past the last 32-row block) start from the same fill on both sides."""
import ctypes as C

import pytest
import torch

gpu = pytest.mark.gpu
K768 = 768
GUARD = 64          # floats on each side of y / dx: a multiple of 4, the kernels store 16 B
SENT = 12345.5
EPS = 1e-5


def _bits(t):
    return t.contiguous().view(torch.int32) if t.element_size() == 4 else t.contiguous().view(torch.int16)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), what


def _inputs(rows, Cc, variant, seed=0):
    """CPU tensors.  plain: non-trivial gamma / beta; hostile: one gamma of 1e24 (every result row carries a 1e24-sized entry:
    the fp32 sum of squares overflows, the pack pass's double does not) and a 1e25-sized dx_add entry; zero: beta = 0 and an
    all-zero input / gradient row (an all-zero result row: exponent of a zero maximum)."""
    g = torch.Generator().manual_seed(seed + rows)
    x = torch.randn(rows, Cc, generator=g) * 3.0 + 0.5
    dy = torch.randn(rows, Cc, generator=g)
    add = torch.randn(rows, Cc, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(Cc, generator=g)
    beta = 0.2 * torch.randn(Cc, generator=g)
    if variant == "hostile":
        gamma[5] = 1e24
        add[rows // 2, 7] = -1e25
        x[rows - 1] *= 1e15
    if variant == "zero":
        beta.zero_()
        x[rows // 3].zero_()
        dy[rows // 3].zero_()
        add[rows // 3].zero_()
    return x, dy, add, gamma, beta


def test_inputs_are_finite():
    """CPU: the hostile inputs stay finite where the kernels need them finite (inputs, LayerNorm statistics in fp32)."""
    for variant in ("plain", "hostile", "zero"):
        for rows in (1, 33, 300):
            x, dy, add, gamma, beta = _inputs(rows, K768, variant)
            for t in (x, dy, add, gamma, beta):
                assert torch.isfinite(t).all()
            var = x.var(dim=1, unbiased=False)
            assert torch.isfinite(var).all() and torch.isfinite(1.0 / torch.sqrt(var + EPS)).all()
            assert torch.equal(x, _inputs(rows, K768, variant)[0])


class _PackBufs:
    def __init__(self, rows, Cc, row_off, dev):
        from semivl_amd import ops
        self.prow = ops.planes_rows(row_off + rows)
        self.buf = torch.full((Cc // 16 * self.prow * 32,), 3.0, dtype=torch.float16, device=dev)
        self.sexp = torch.full((self.prow,), 77, dtype=torch.int32, device=dev)
        self.rnorm = torch.full((self.prow,), SENT, dtype=torch.float32, device=dev)
        self.amax = torch.full((1,), 99, dtype=torch.int32, device=dev)

    def same(self, other, what):
        for n in ("buf", "sexp", "rnorm", "amax"):
            _same(getattr(self, n), getattr(other, n), f"{what}: {n}")


def _guarded(rows, Cc, dev):
    buf = torch.full((rows * Cc + 2 * GUARD,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + rows * Cc].view(rows, Cc)


def _guard_ok(buf, n):
    ref = torch.full((GUARD,), SENT, dtype=torch.float32, device=buf.device)
    return torch.equal(buf[:GUARD], ref) and torch.equal(buf[GUARD + n:], ref)


def _split(res, pb, row_off):
    from semivl_amd import ops, lib as L
    rows, Cc = res.shape
    L.check(L.load().svl_split_planes_f16x2(ops._p(res), res.stride(0), 1, rows, Cc, ops._p(pb.buf), pb.prow, row_off,
                                            ops._p(pb.sexp), ops._p(pb.rnorm), ops._p(pb.amax), ops._st()), "split")


def _fwd_ref(x, gamma, beta, row_off, want_y):
    from semivl_amd import ops, lib as L
    rows, Cc = x.shape
    lib = L.load()
    stats = torch.full((rows, 2), SENT, device=x.device)
    pb = _PackBufs(rows, Cc, row_off, x.device)
    if want_y:
        ybuf, y = _guarded(rows, Cc, x.device)
        L.check(lib.svl_layernorm_fwd(ops._p(x), ops._p(gamma), ops._p(beta), EPS, rows, Cc, ops._p(y), ops._p(stats), ops._st()), "ln")
        _split(y, pb, row_off)
        return ybuf, stats, pb
    assert row_off == 0
    L.check(lib.svl_layernorm_fwd_planes_f16x2(ops._p(x), ops._p(gamma), ops._p(beta), EPS, rows, Cc, None, ops._p(stats),
                                               ops._p(pb.buf), pb.prow, ops._p(pb.sexp), ops._p(pb.rnorm), ops._st()), "lnp")
    return None, stats, pb


def _fwd_new(x, gamma, beta, row_off, want_y):
    from semivl_amd import ops, lib as L
    rows, Cc = x.shape
    stats = torch.full((rows, 2), SENT, device=x.device)
    pb = _PackBufs(rows, Cc, row_off, x.device)
    ybuf, y = _guarded(rows, Cc, x.device) if want_y else (None, None)
    L.check(L.load().svl_layernorm_fwd_pack_f16x2(ops._p(x), ops._p(gamma), ops._p(beta), EPS, rows, Cc, ops._p(y), ops._p(stats),
                                                  ops._p(pb.buf), pb.prow, row_off, ops._p(pb.sexp), ops._p(pb.rnorm),
                                                  0 if want_y else 1, ops._p(pb.amax) if want_y else None, ops._st()), "lnpack")
    return ybuf, stats, pb


FWD_CASES = [(1, "plain", 0), (33, "plain", 0), (256, "plain", 0), (300, "plain", 0), (300, "hostile", 0), (33, "zero", 0),
             (300, "plain", 64), (17, "hostile", 32)]


# (the planes-only reference kernel has no row offset)
FWD_PARAMS = [c + (True,) for c in FWD_CASES] + [c + (False,) for c in FWD_CASES if c[2] == 0]


@gpu
@pytest.mark.parametrize("rows,variant,row_off,want_y", FWD_PARAMS)
def test_layernorm_fwd_pack_bits(dev, rows, variant, row_off, want_y):
    x, _, _, gamma, beta = (t.to(dev) for t in _inputs(rows, K768, variant))
    ry, rst, rpb = _fwd_ref(x, gamma, beta, row_off, want_y)
    ry2, rst2, rpb2 = _fwd_ref(x, gamma, beta, row_off, want_y)
    rpb.same(rpb2, "reference sequence is deterministic")
    outs = [_fwd_new(x, gamma, beta, row_off, want_y) for _ in range(2)]
    for ny, nst, npb in outs:
        _same(nst, rst, "stats")
        if want_y:
            _same(ny, ry, "y and its guard band")
            assert _guard_ok(ny, rows * K768)
            npb.same(rpb, "planes / sexp / rnorm / amax, padding rows included")
        else:
            for n in ("buf", "sexp", "rnorm"):
                _same(getattr(npb, n), getattr(rpb, n), n)
            assert int(npb.amax) == 99, "tensor_amax off: the word is not touched"
    if want_y and variant != "hostile":
        assert torch.isfinite(outs[0][0]).all()


def _bwd_ref(dy, x, stats, gamma, add, row_off):
    from semivl_amd import ops, lib as L
    rows, Cc = x.shape
    pb = _PackBufs(rows, Cc, row_off, x.device)
    dbuf, dx = _guarded(rows, Cc, x.device)
    L.check(L.load().svl_layernorm_bwd(ops._p(dy), ops._p(x), ops._p(stats), ops._p(gamma), rows, Cc, ops._p(add), ops._p(dx),
                                       None, None, ops._st()), "lnb")
    _split(dx, pb, row_off)
    return dbuf, pb


def _bwd_new(dy, x, stats, gamma, add, row_off):
    from semivl_amd import ops, lib as L
    rows, Cc = x.shape
    pb = _PackBufs(rows, Cc, row_off, x.device)
    dbuf, dx = _guarded(rows, Cc, x.device)
    L.check(L.load().svl_layernorm_bwd_pack_f16x2(ops._p(dy), ops._p(x), ops._p(stats), ops._p(gamma), rows, Cc, ops._p(add),
                                                  ops._p(dx), ops._p(pb.buf), pb.prow, row_off, ops._p(pb.sexp),
                                                  ops._p(pb.rnorm), ops._p(pb.amax), ops._st()), "lnbpack")
    return dbuf, pb


@gpu
@pytest.mark.parametrize("rows,variant,row_off", FWD_CASES)
@pytest.mark.parametrize("with_add", [True, False])
def test_layernorm_bwd_pack_bits(dev, rows, variant, row_off, with_add):
    from semivl_amd import ops
    x, dy, add, gamma, beta = (t.to(dev) for t in _inputs(rows, K768, variant))
    _, stats = ops.layernorm_fwd(x, gamma, beta, EPS)
    add = add if with_add else None
    rbuf, rpb = _bwd_ref(dy, x, stats, gamma, add, row_off)
    rbuf2, rpb2 = _bwd_ref(dy, x, stats, gamma, add, row_off)
    _same(rbuf, rbuf2, "reference sequence is deterministic")
    rpb.same(rpb2, "reference sequence is deterministic")
    for _ in range(2):
        nbuf, npb = _bwd_new(dy, x, stats, gamma, add, row_off)
        _same(nbuf, rbuf, "dx and its guard band")
        assert _guard_ok(nbuf, rows * K768)
        npb.same(rpb, "planes / sexp / rnorm / amax, padding rows included")


@gpu
@pytest.mark.parametrize("Cc", [768, 512])
@pytest.mark.parametrize("want_wgrad", [False, True])
def test_ops_layernorm_routes(dev, Cc, want_wgrad):
    """ops.layernorm_fwd / layernorm_bwd with planes=True: C = 768 on the one-pass kernels, C = 512 and the weight-gradient
    form on the two-kernel sequence -- the same bits as that sequence either way, dgamma / dbeta included."""
    from semivl_amd import ops
    if ops.PLANES_FMT != "h2":
        pytest.skip("SVL_PLANES_FMT=b3 A/B run: other kernels serve these calls")
    rows = 300
    x, dy, add, gamma, beta = (t.to(dev) for t in _inputs(rows, Cc, "plain"))

    def planes_same(a, b):
        nb = (rows + 31) // 32 * 32
        _same(a.sexp[:nb], b.sexp[:nb], "sexp")
        _same(a.rnorm[:nb], b.rnorm[:nb], "rnorm")
        per = a.prow * 32
        for kg in range(Cc // 16):
            _same(a.buf[kg * per:kg * per + nb * 32], b.buf[kg * per:kg * per + nb * 32], "planes")

    y, st, pl = ops.layernorm_fwd(x, gamma, beta, EPS, planes=True, want_y=True)
    y0, st0 = ops.layernorm_fwd(x, gamma, beta, EPS)
    _same(y, y0, "y")
    _same(st, st0, "stats")
    planes_same(pl, ops.split_planes(y0))
    if pl.amax is not None:
        assert int(pl.amax) == int(y0.abs().max().view(torch.int32))
    res = ops.layernorm_bwd(dy, x, st, gamma, dx_add=add, want_wgrad=want_wgrad, planes=True)
    ref = ops.layernorm_bwd(dy, x, st, gamma, dx_add=add, want_wgrad=want_wgrad)
    ref = ref if want_wgrad else (ref,)
    for a, b in zip(res[:-1], ref):
        _same(a, b, "dx / dgamma / dbeta")
    planes_same(res[-1], ops.split_planes(ref[0]))


def _amax_word(m):
    return int(m.abs().max().view(torch.int32))     # (exact: a maximum has no rounding; what an operand-maximum pass leaves)


@gpu
@pytest.mark.parametrize("rows,Kc,ld", [(300, 768, 768), (300, 768, 800), (72, 768, 768), (1, 768, 768), (33, 2304, 2304)])
def test_split_planes_tensor_amax(dev, rows, Kc, ld):
    """rows = 300: the maximum sits in the last, partial 32-row block; rows = 72: three row blocks, k-split launch (ysplit > 1);
    ld > K: a strided source, its gaps holding larger values that must not count."""
    g = torch.Generator().manual_seed(rows)
    full = (torch.randn(rows, ld, generator=g)).to(dev)
    if ld > Kc:
        full[:, Kc:] = 1e6
    m = full[:, :Kc]
    m[rows - 1, Kc - 3] = -37.25
    pb = _PackBufs(rows, Kc, 0, dev)
    _split(m, pb, 0)
    assert int(pb.amax) == _amax_word(m) == int(torch.tensor(37.25).view(torch.int32))
    pb0 = _PackBufs(rows, Kc, 0, dev)
    pb0.amax = None
    _split(m, pb0, 0)
    for n in ("buf", "sexp", "rnorm"):
        _same(getattr(pb, n), getattr(pb0, n), n + " does not depend on tensor_amax")
    z = _PackBufs(rows, Kc, 0, dev)
    _split(torch.zeros(rows, Kc, device=dev), z, 0)
    assert int(z.amax) == 0


@gpu
@pytest.mark.parametrize("Kk,h2", [(1152, True), (1024, False)])
def test_matmul_tn_with_supplied_maxima(dev, Kk, h2):
    """M = 2304, N = 768, K = 1152 in mode 6: 4.08 GFLOP >= the 4 GFLOP floor of the fp16 x 2 form, and 6.9 us of saved matrix
    time against 1.5 x 3.5 us for the two maximum passes (the constants of svl_gemm_f32's dense branch).  K = 1024 is below
    the floor: the maxima are ignored and the launch stays on the bf16 x 3 form."""
    from semivl_amd import ops, lib as L
    lib = L.load()
    mode0 = ops.get_gemm_emulation()
    ops.set_gemm_emulation(6)
    try:
        g = torch.Generator().manual_seed(Kk)
        a = (torch.randn(Kk, 2304, generator=g) * 0.01).to(dev)
        b = (torch.randn(Kk, 768, generator=g) * 2.0).to(dev)
        pa, pb = ops.split_planes(a, want_amax=True, fmt="h2"), ops.split_planes(b, want_amax=True, fmt="h2")
        assert int(pa.amax) == _amax_word(a) and int(pb.amax) == _amax_word(b)
        n0 = lib.svl_absmax_launches()
        ref = ops.matmul_tn(a, b)
        path_ref = lib.svl_last_gemm_path()
        n1 = lib.svl_absmax_launches()
        out = ops.matmul_tn(a, b, a_amax=pa.amax, b_amax=pb.amax)
        path_new = lib.svl_last_gemm_path()
        n2 = lib.svl_absmax_launches()
        one = ops.matmul_tn(a, b, a_amax=pa.amax)
        n3 = lib.svl_absmax_launches()
    finally:
        ops.set_gemm_emulation(mode0)
    _same(out, ref, "supplied maxima change no bit")
    _same(one, ref, "one supplied maximum changes no bit")
    assert path_ref == path_new == (4 if h2 else 1)
    assert (n1 - n0, n2 - n1, n3 - n2) == ((2, 0, 1) if h2 else (0, 0, 0))
    assert torch.allclose(ref, a.double().t().mm(b.double()).float(), rtol=1e-4, atol=1e-4)


@gpu
def test_matmul_tn_gelu_with_supplied_maximum(dev):
    """The producer branch of svl_gemm_f32 (B = gelu(h) while staging) at M = 768, N = 3072, K = 1152 in mode 6: 5.4 GFLOP,
    9.2 us of saved matrix time against 1.5 x 4.4 us of maximum passes.  A supplied a_amax replaces the pass over A (the
    producer's transformed B operand keeps its own); the result keeps every bit."""
    from semivl_amd import ops, lib as L
    lib = L.load()
    mode0 = ops.get_gemm_emulation()
    ops.set_gemm_emulation(6)
    try:
        g = torch.Generator().manual_seed(7)
        a = (torch.randn(1152, 768, generator=g) * 0.01).to(dev)
        h = (torch.randn(1152, 3072, generator=g) * 2.0).to(dev)
        pa = ops.split_planes(a, want_amax=True, fmt="h2")
        assert int(pa.amax) == _amax_word(a)
        n0 = lib.svl_absmax_launches()
        ref = ops.matmul_tn_gelu(a, h)
        path_ref = lib.svl_last_gemm_path()
        n1 = lib.svl_absmax_launches()
        out = ops.matmul_tn_gelu(a, h, a_amax=pa.amax)
        path_new = lib.svl_last_gemm_path()
        n2 = lib.svl_absmax_launches()
    finally:
        ops.set_gemm_emulation(mode0)
    _same(out, ref, "a supplied maximum changes no bit")
    assert path_ref == path_new == 4
    assert (n1 - n0, n2 - n1) == (1, 0)
