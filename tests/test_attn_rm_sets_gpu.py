"""GPU: the fp16 x 2 attention on ROW-MAJOR operand sets only (transposed fragments formed while reading LDS) and the backward
on the sets its forward kept -- bit for bit what the previous sequence (ops.attention_tr_sets(True): transposed sets packed and
read, the backward packing q, k, v again) computes.

Shapes: Bn = 2, H = 2, head dim 64; T = 33 (shorter than one key tile), 64 (exact tile), 65 (the 1025 case in small: a last key
tile of one key, Tp = 128), 257 (one leftover query row: the tail kernels run)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BN, H, D = 2, 2, 64
E = H * D
TS = [33, 64, 65, 257]
# the bound tests/test_ops_gpu.py::test_fused_attention_split_emulation holds the fp16 x 2 kernels to, restated: the error level
# (root mean square vs float64) <= 1.2 x the exact fp32 kernels' + a tenth of the slack, the largest error <= 2 x theirs + slack
EMU6_ERR_FACTOR = 1.2


@pytest.fixture
def h2():
    """The fp16 x 2 attention kernels (emulation mode 6) for one test; the operand-set switch is restored whatever happens."""
    from semivl_amd import ops
    ops.set_gemm_emulation(6)
    assert ops.attention_h2()
    keep = ops.attention_tr_sets()
    yield ops
    ops.attention_tr_sets(keep)
    ops.set_gemm_emulation(0)


def _inputs(dev, T, zeros):
    g = torch.Generator(device="cpu").manual_seed(1000 + T)
    qkv = torch.randn(BN * T, 3 * E, generator=g)
    qkv[:, :2 * E] *= 2.0
    do = torch.randn(BN * T, E, generator=g)
    if zeros:   # the first 64 rows of a slice are zeros: the pack's exponent guess fails and it takes its second attempt
        n = min(64, T)
        qkv[:n, E + D:E + 2 * D] = 0.0        # k of image 0, head 1
        qkv[T:T + n, 2 * E:2 * E + D] = 0.0   # v of image 1, head 0
        do[:n, D:2 * D] = 0.0                 # dO of image 0, head 1
    return qkv.to(dev), do.to(dev)


def _run(ops, qkv, do, T, sets=False):
    if sets:
        out, lse, ws = ops.attention_fwd(qkv, BN, T, H, keep_sets=True)
        return out, lse, ops.attention_bwd(do, qkv, out, lse, BN, T, H, sets=ws)
    out, lse = ops.attention_fwd(qkv, BN, T, H)
    return out, lse, ops.attention_bwd(do, qkv, out, lse, BN, T, H)


@pytest.mark.parametrize("zeros", [False, True])
@pytest.mark.parametrize("T", TS)
def test_rm_sets_equal_the_tr_sequence_bit_for_bit(dev, h2, T, zeros):
    ops = h2
    qkv, do = _inputs(dev, T, zeros)
    ops.attention_tr_sets(False)
    new = _run(ops, qkv, do, T)
    kept = _run(ops, qkv, do, T, sets=True)
    assert ops.attention_tr_sets(True) is False
    old = _run(ops, qkv, do, T)
    assert ops.attention_fwd(qkv, BN, T, H, keep_sets=True)[2] is None     # nothing to keep under the switch
    assert ops.attention_tr_sets(False) is True
    for what, a, b, c in zip(("out", "lse", "dqkv"), new, old, kept):
        assert torch.isfinite(b).all(), what
        assert torch.equal(a, b), (what, "rm sets vs tr sets", float((a - b).abs().max()))
        assert torch.equal(c, b), (what, "kept sets vs tr sets", float((c - b).abs().max()))


@pytest.mark.parametrize("T", TS)
def test_backward_reads_the_kept_sets(dev, h2, T):
    """sets= from the forward of the same qkv: the same bits as without; from another qkv: another result (the argument is used)."""
    ops = h2
    ops.attention_tr_sets(False)
    qkv, do = _inputs(dev, T, False)
    out, lse, ws = ops.attention_fwd(qkv, BN, T, H, keep_sets=True)
    assert ws is not None and ws.dtype == torch.uint8
    ref = ops.attention_bwd(do, qkv, out, lse, BN, T, H)
    keep = ws.clone()
    assert torch.equal(ops.attention_bwd(do, qkv, out, lse, BN, T, H, sets=ws), ref)
    assert torch.equal(ws, keep)                                            # read only
    other = _inputs(dev, T, True)[0] * 1.5
    ws2 = ops.attention_fwd(other, BN, T, H, keep_sets=True)[2]
    assert not torch.equal(ops.attention_bwd(do, qkv, out, lse, BN, T, H, sets=ws2), ref)


def _codes(T, seed):
    """T words of {-1, +1}^32 with pairwise Hamming distance >= 8 (greedy, deterministic)."""
    rng = np.random.RandomState(seed)
    words = np.zeros((0, 32), np.int64)
    while len(words) < T:
        c = rng.randint(0, 2, size=(1, 32)) * 2 - 1
        if len(words) == 0 or ((words != c).sum(1) >= 8).all():
            words = np.concatenate([words, c])
    return torch.from_numpy(words)


@pytest.mark.parametrize("T", TS)
def test_fragment_order_on_exact_integer_data(dev, h2, T):
    """Small integers (|x| <= 4): every scaled operand is one fp16 term and every MFMA sum an exact fp32 integer.  One key
    dominates each query's softmax with logit 0 against <= -32 for every other key (k = 4 (code, -1), q = 4 (code of its key,
    +1), codes 8 sign flips apart): P is exactly 1 there (lse = 0 exactly) and rounds to 0 elsewhere, so out = v of that key and
    dV = P^T dO = dO of the one query that chose the key, exactly -- any fragment whose (token, channel) order were wrong would
    move integers to other places.  The dominant keys are a permutation of the tokens spread over all key tiles.

    Where the sums are integers: lse and dV everywhere; `out` for the queries whose dominant key lies in the FIRST 64-key tile
    (the running maximum is final from that tile on and every later probability rounds to 0 in fp16), with them dQ = 0 of
    those queries and dK = 0 of the keys 0..63.  A query whose dominant key comes in a later tile carries the earlier tiles'
    sum, rescaled by 2^-46, in its accumulator when the dominant product arrives: a non-integer far below half an ulp, which
    the MFMA's addition does not round to nearest.  Measured at T = 65 and 257, identical on both operand-set sequences (the
    parent's included): about a sixth of those queries' `out` values (45 of 256 at T = 65, 9205 at T = 257) come out one
    ulp short in magnitude (4 - 2^-22 for 4; largest error 2.4e-7), D = rowsum(dO O) then misses dP by an ulp of D and dQ of
    the query / dK of its key are 2^-20 .. 2.9e-6 instead of 0 (the exact fp32 kernels round that addition to nearest and
    stay exact: 3e-13 from float64).  Those are no integer combinations.  `out` as a whole is held to the split emulation's
    bound (EMU6_ERR_FACTOR above) against the exact fp32 kernels on the same data (rms 5.9e-8 against 1e-7, largest 2.4e-7
    against 1e-6 at T = 257), and every value to one ulp of its accumulator, 2^-23 |v|: the one addition that meets the
    remainder may truncate, the products before and after it are zeros and 1 / l = 2^-7 is exact.  dQ and dK there are not
    zeros because D = rowsum(dO O) is not dP any more: with Dabs = the largest sum_d |dO_d v_d| of a row, the 64 products
    dO_d O_d are off by <= 2^-23 Dabs together, their roundings add <= 2^-24 Dabs and the 7 fp32 additions of the row sum
    <= 2^-24 Dabs each, so |dP - D| <= 10 x 2^-24 Dabs; P = 1, and dQ = dS k / 8, dK = dS q / 8 with |k|, |q| = 4 (1 % on
    top for the split of dS).  The K and Q fragments' order does not show in these zeros; the bit equality above holds it."""
    ops = h2
    ops.attention_tr_sets(False)
    g = torch.Generator(device="cpu").manual_seed(7 + T)
    qkv = torch.zeros(BN, T, 3, H, D)
    pick = torch.empty(BN, H, T, dtype=torch.long)
    for b in range(BN):
        for h in range(H):
            c = _codes(T, 100 * b + h + T).float()
            jstar = (7 * torch.arange(T) + 3 + 11 * b + 5 * h) % T          # gcd(7, T) = 1 for every T here
            pick[b, h] = jstar
            qkv[b, :, 0, h, :32], qkv[b, :, 0, h, 32:] = 4 * c[jstar], 4.0
            qkv[b, :, 1, h, :32], qkv[b, :, 1, h, 32:] = 4 * c, -4.0
    v = torch.randint(1, 5, (BN, T, H, D), generator=g).float() * (torch.randint(0, 2, (BN, T, H, D), generator=g) * 2 - 1)
    qkv[:, :, 2] = v
    do = torch.randint(-4, 5, (BN, T, H, D), generator=g).float()
    qkv_d, do_d = qkv.reshape(BN * T, 3 * E).to(dev), do.reshape(BN * T, E).to(dev)
    # float64 restatement
    q64, k64, v64 = [qkv[:, :, i].double().permute(0, 2, 1, 3) for i in range(3)]       # [BN, H, T, D]
    p64 = ((q64 @ k64.transpose(-1, -2)) / 8.0).softmax(-1)
    out64 = (p64 @ v64).permute(0, 2, 1, 3).reshape(BN * T, E)
    dv64 = (p64.transpose(-1, -2) @ do.double().permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(BN * T, E)
    assert int((p64 > 0.5).sum()) == BN * H * T and (out64 - out64.round()).abs().max() < 1e-9
    assert (dv64 - dv64.round()).abs().max() < 1e-9                                      # integer combinations throughout
    # [BN * T, E] masks of the integer sums: queries whose dominant key is in key tile 0; keys of tile 0
    first_q = (pick < 64).permute(0, 2, 1).reshape(BN * T, H, 1).expand(-1, -1, D).reshape(BN * T, E)
    first_k = (torch.arange(T) < 64).repeat(BN).view(BN * T, 1).expand(-1, E)
    assert int((~first_q).sum()) == BN * H * max(T - 64, 0) * D      # (the dominant keys are a permutation)
    # the float64 gradient itself for the bound (dQ, dK are ~1e-12 there, not 0)
    qd = qkv.reshape(BN * T, 3 * E).double().requires_grad_(True)
    qa, ka, va = [t.reshape(BN, T, H, D).transpose(1, 2) for t in qd.view(BN, T, 3 * E).split(E, dim=2)]
    oa = (((qa * D ** -0.5) @ ka.transpose(-1, -2)).softmax(-1) @ va).transpose(1, 2).reshape(BN * T, E)
    (g64,) = torch.autograd.grad(oa, qd, do.reshape(BN * T, E).double())
    assert float((oa.detach() - out64).abs().max()) < 1e-9 and float((g64[:, 2 * E:] - dv64).abs().max()) < 1e-9
    refs = (out64, g64, torch.zeros(BN * H * T, dtype=torch.float64))
    dabs = float((do.reshape(BN * T, H, D).double().abs() * out64.round().view(BN * T, H, D).abs()).sum(-1).max())
    dqk_bound = 0.125 * 4.0 * 1.01 * 10 * 2.0 ** -24 * dabs

    def errors(out, dqkv, lse):
        errs = [a.cpu().double() - b for a, b in zip((out, dqkv, lse), refs)]
        return [float(e.abs().max()) for e in errs], [float(e.pow(2).mean().sqrt()) for e in errs]

    ops.set_gemm_emulation(0)                # the exact fp32 kernels on the same data: the bound's yardstick
    assert not ops.attention_h2()
    out0, lse0 = ops.attention_fwd(qkv_d, BN, T, H)
    max0, rms0 = errors(out0, ops.attention_bwd(do_d, qkv_d, out0, lse0, BN, T, H), lse0)
    ops.set_gemm_emulation(6)
    assert ops.attention_h2()
    for tr in (False, True):      # (the previous sequence meets the same statements: they are properties of the arithmetic)
        ops.attention_tr_sets(tr)
        out, lse, ws = ops.attention_fwd(qkv_d, BN, T, H, keep_sets=True)
        dqkv = ops.attention_bwd(do_d, qkv_d, out, lse, BN, T, H, sets=ws)
        max6, rms6 = errors(out, dqkv, lse)
        print(f"RM_SETS_EXACT T{T} tr{int(tr)}: max " + " ".join(f"{a:.2e}/{b:.2e}" for a, b in zip(max0, max6)) +
              " rms " + " ".join(f"{a:.2e}/{b:.2e}" for a, b in zip(rms0, rms6)))
        o, dq, dk = out.cpu().double(), dqkv[:, :E].cpu(), dqkv[:, E:2 * E].cpu()
        assert torch.equal(o[first_q], out64.round()[first_q]), ("out", tr)
        assert torch.equal(lse.cpu(), torch.zeros(BN * H * T)), ("lse", tr)
        assert torch.equal(dqkv[:, 2 * E:].cpu().double(), dv64.round()), ("dV", tr)
        assert torch.equal(dq[first_q], torch.zeros(int(first_q.sum()))), ("dQ: dS = P (dP - D) = 0 exactly", tr)
        assert torch.equal(dk[first_k], torch.zeros(int(first_k.sum()))), ("dK: dS = P (dP - D) = 0 exactly", tr)
        # out (whole tensor; dV and lse are exact above): the split emulation's bound against the exact fp32 kernels
        assert rms6[0] <= EMU6_ERR_FACTOR * rms0[0] + 0.1 * 1e-6, ("out", "rms", tr, rms0[0], rms6[0])
        assert max6[0] <= 2.0 * max0[0] + 1e-6, ("out", "max", tr, max0[0], max6[0])
        # ... and no further than one ulp of the accumulator from the integer: a misplaced integer is off by >= 1
        assert bool(((o - out64.round()).abs() <= 2.0 ** -23 * out64.round().abs()).all()), ("out, one ulp", tr)
        # dQ, dK where D carries the short `out` values: |dQ|, |dK| <= 0.125 x 4 x |dP - D| (see the docstring)
        worst = float(torch.maximum(dq.abs().max(), dk.abs().max()))
        print(f"RM_SETS_EXACT T{T} tr{int(tr)}: dQ, dK largest {worst:.2e}, bound {dqk_bound:.2e}")
        assert worst <= dqk_bound, ("dQ, dK", tr, worst, dqk_bound)
    ops.attention_tr_sets(False)


@pytest.mark.parametrize("T", TS)
def test_integer_data_without_a_dominant_key_keeps_the_split_emulation_bound(dev, h2, T):
    """Random small integers: nothing is an integer combination any more; out, dqkv and lse keep the bound the split emulation
    is held to against the exact fp32 kernels (see EMU6_ERR_FACTOR above)."""
    ops = h2
    ops.attention_tr_sets(False)
    g = torch.Generator(device="cpu").manual_seed(77 + T)
    qkv = torch.randint(-4, 5, (BN * T, 3 * E), generator=g).float().to(dev)
    do = torch.randint(-4, 5, (BN * T, E), generator=g).float().to(dev)
    qd = qkv.double().requires_grad_(True)
    q, k, v = [t.reshape(BN, T, H, D).transpose(1, 2) for t in qd.view(BN, T, 3 * E).split(E, dim=2)]
    sc = (q * D ** -0.5) @ k.transpose(-1, -2)
    o64 = (sc.softmax(-1) @ v).transpose(1, 2).reshape(BN * T, E)
    (g64,) = torch.autograd.grad(o64, qd, do.double())
    lse64 = torch.logsumexp(sc, -1).detach()
    res, rms = {}, {}
    for mode in (0, 6):
        ops.set_gemm_emulation(mode)
        assert ops.attention_h2() == (mode == 6)
        out, lse, ws = ops.attention_fwd(qkv, BN, T, H, keep_sets=True)
        dqkv = ops.attention_bwd(do, qkv, out, lse, BN, T, H, sets=ws)
        errs = (out.double() - o64.detach(), dqkv.double() - g64, lse.view(BN, H, T).double() - lse64)
        res[mode] = tuple(float(e.abs().max()) for e in errs)
        rms[mode] = tuple(float(e.pow(2).mean().sqrt()) for e in errs)
    lse_ulp = 1.2e-7 * float(lse64.abs().max())
    print(f"RM_SETS_GATE T{T}: max " + " ".join(f"{a:.2e}/{b:.2e}" for a, b in zip(res[0], res[6])) +
          " rms " + " ".join(f"{a:.2e}/{b:.2e}" for a, b in zip(rms[0], rms[6])))
    for i, (what, slack) in enumerate((("out", 1e-6), ("dqkv", 1e-6), ("lse", 2 * lse_ulp))):
        assert rms[6][i] <= EMU6_ERR_FACTOR * rms[0][i] + 0.1 * slack, (what, "rms", rms[0][i], rms[6][i])
        assert res[6][i] <= 2.0 * res[0][i] + slack, (what, "max", res[0][i], res[6][i])


@pytest.mark.parametrize("T", TS)
def test_workspace_sizes_and_refusals(dev, h2, T):
    """3 sets forward, 4 backward, 1 on kept sets (7 backward under the switch); a workspace one byte short is refused."""
    from semivl_amd import lib as L
    ops = h2
    lib = L.load()
    ops.attention_tr_sets(False)
    Tp = (T + 63) // 64 * 64
    S = BN * H * Tp * 256
    small = 2 * 1024                                   # exponents, norms: B H 16 bytes each, rounded up to 1 KiB
    pairs = (BN * H * Tp * 8 + 1023) // 1024 * 1024 + 1024
    n = [lib.svl_attention_h2_ws_bytes(BN, T, H, m) for m in (0, 1, 2)]
    assert n == [3 * S + small, 4 * S + small + pairs, S + small + pairs]
    assert lib.svl_attention_h2_ws_bytes(BN, T, H, 3) == 0
    ops.attention_tr_sets(True)
    assert lib.svl_attention_h2_ws_bytes(BN, T, H, 1) == 7 * S + small + pairs
    ops.attention_tr_sets(False)
    qkv, do = _inputs(dev, T, False)
    out, lse, sets = ops.attention_fwd(qkv, BN, T, H, keep_sets=True)
    dqkv, dsum = torch.empty_like(qkv), ops.empty(BN * H * T, device=dev)
    ws = torch.empty(n[1] + 1024, dtype=torch.uint8, device=dev)
    p, wp, sp = ops._p, ops._ws_ptr(ws), ops._ws_ptr(sets)
    INVALID = -1
    assert lib.svl_attention_fwd_h2(p(qkv), BN, T, H, p(out), p(lse), None, 0, wp, n[0] - 1, None) == INVALID
    assert "workspace" in L.last_error()
    assert lib.svl_attention_bwd_h2(p(qkv), p(out), p(do), p(lse), BN, T, H, p(dsum), p(dqkv), None, 0, wp, n[1] - 1, None) == INVALID
    args = (p(qkv), p(out), p(do), p(lse), BN, T, H, p(dsum), p(dqkv))
    assert lib.svl_attention_bwd_h2_sets(*args, sp, n[0], wp, n[2] - 1, None) == INVALID
    assert lib.svl_attention_bwd_h2_sets(*args, sp, n[0] - 1, wp, n[2], None) == INVALID
    assert lib.svl_attention_bwd_h2_sets(*args, None, n[0], wp, n[2], None) == INVALID
    ops.attention_tr_sets(True)
    assert lib.svl_attention_bwd_h2_sets(*args, sp, n[0], wp, n[1], None) == INVALID      # no kept sets under the switch
    ops.attention_tr_sets(False)
    torch.cuda.synchronize()
