"""GPU: the kernels of csrc/text.hip (svl_text_embed_f32, svl_causal_attn_fwd_f32, svl_quickgelu_f32, svl_gather_rows_f32,
svl_segment_mean_f32) against torch on the host: bit-equal where the kernel only moves or adds once, float64 bounds elsewhere.
Output buffers are carved out of larger ones filled with a sentinel: the guard bands on both sides must stay intact."""
import ctypes as C
import itertools

import pytest
import torch

import text_ref as R

pytestmark = pytest.mark.gpu

SENT = -12345.5
U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


def _lib():
    import semivl_amd.lib as L
    return L, L.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def guarded(numel, dev, dtype=torch.float32, guard=64):
    """(whole buffer, the view of `numel` elements `guard` elements in)"""
    buf = torch.full((numel + 2 * guard,), SENT, dtype=dtype, device=dev) if dtype.is_floating_point else \
        torch.full((numel + 2 * guard,), -777, dtype=dtype, device=dev)
    return buf, buf[guard:guard + numel]


def guards_intact(buf, numel, guard=64):
    s = SENT if buf.dtype.is_floating_point else -777
    return bool((buf[:guard] == s).all()) and bool((buf[guard + numel:] == s).all())


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- svl_text_embed_f32 --------------------------------------------------------------------------------------------------
def test_text_embed_bit_equal_with_guards(dev):
    L_, lib = _lib()
    g = torch.Generator().manual_seed(0)
    for n, Lc, W, V in itertools.product((1, 3), (1, 9, 77), (64, 128, 512), (3, 40)):
        table, pos = torch.randn(V, W, generator=g), torch.randn(Lc, W, generator=g)
        tok = torch.randint(0, V, (n, Lc), generator=g)
        want = table[tok] + pos[None]
        tok_d, table_d, pos_d = tok.to(dev), table.to(dev), pos.to(dev)
        for guard in (64, 61):          # 61: x is off a 16-byte boundary, the scalar path
            xb, x = guarded(n * Lc * W, dev, guard=guard)
            eb, e = guarded(n, dev, torch.int32)
            rc = lib.svl_text_embed_f32(_p(tok_d), _p(table_d), _p(pos_d), n, Lc, V, W, _p(x), _p(e), _st())
            assert rc == 0, L_.last_error()
            assert torch.equal(bits(x.cpu()), bits(want.reshape(-1))), (n, Lc, W, V, guard)
            assert e.cpu().tolist() == tok.argmax(-1).tolist(), (n, Lc, W, V)
            assert guards_intact(xb, n * Lc * W, guard) and guards_intact(eb, n)


def test_text_embed_eot_is_the_first_maximum(dev):
    from semivl_amd import ops
    V, W = 40, 64
    g = torch.Generator().manual_seed(1)
    table = torch.randn(V, W, generator=g).to(dev)
    for Lc in (1, 2, 9, 64, 65, 77, 192):
        pos = torch.randn(Lc, W, generator=g).to(dev)
        rows = [torch.randint(0, V - 1, (Lc,), generator=g) for _ in range(6)]
        rows[0][0] = V - 1                                    # the maximum at position 0
        rows[1][:] = 7                                        # every position ties: the first one
        rows[2][Lc - 1] = V - 1                               # at the last position
        rows[3][Lc // 2] = V - 1
        rows[3][Lc - 1] = V - 1                               # repeated: the earlier one
        rows[4][:] = 0
        rows[5][Lc // 3] = V - 1
        if Lc // 3 + 64 < Lc:
            rows[5][Lc // 3 + 64] = V - 1                     # repeated 64 apart: the same lane sees both
        tok = torch.stack(rows)
        x, eot = ops.text_embed(tok.to(dev), table, pos)
        assert eot.dtype == torch.int32 and eot.cpu().tolist() == tok.argmax(-1).tolist(), Lc
        assert torch.equal(x.cpu(), (table.cpu()[tok] + pos.cpu()[None]).reshape(-1, W))


def test_text_embed_wrapper_refuses_ids_outside_the_table(dev):
    from semivl_amd import ops
    V, W, Lc = 40, 64, 9
    table, pos = torch.randn(V, W, device=dev), torch.randn(Lc, W, device=dev)
    for bad in (-1, V):
        tok = torch.randint(0, V, (3, Lc))
        tok[1, 4] = bad
        with pytest.raises(ValueError, match=str(bad)):
            ops.text_embed(tok.to(dev), table, pos)
    L_, lib = _lib()
    tok = torch.zeros(1, Lc, dtype=torch.int64, device=dev)
    x, e = torch.empty(Lc * W, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    for args, word in (((None, _p(table), _p(pos), 1, Lc, V, W, _p(x), _p(e)), "tokens"),
                       ((_p(tok), _p(table), _p(pos), 1, Lc, V, W, None, _p(e)), "x is null"),
                       ((_p(tok), _p(table), _p(pos), 1, Lc, 0, W, _p(x), _p(e)), "V 0"),
                       ((_p(tok), _p(table), _p(pos), 0, Lc, V, W, _p(x), _p(e)), "n 0")):
        assert lib.svl_text_embed_f32(*args, _st()) == -1
        assert "svl_text_embed_f32" in L_.last_error() and word in L_.last_error()


# ---- svl_causal_attn_fwd_f32 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lc", [1, 2, 63, 64, 65, 77, 191, 192])
def test_causal_attention(dev, Lc):
    from semivl_amd import ops
    g = torch.Generator().manual_seed(100 + Lc)
    for n, H in itertools.product((1, 3), (1, 2, 8)):
        W = 64 * H
        qkv = torch.randn(n * Lc, 3 * W, generator=g)
        ref = R.causal_attention(qkv, n, Lc, H)
        ob, o = guarded(n * Lc * W, dev)
        out = ops.causal_attn_fwd(qkv.to(dev), n, Lc, H, out=o.view(n * Lc, W))
        got = out.cpu()
        err = (got.double() - ref).abs().max().item()
        print(f"causal attention n={n} H={H} L={Lc}: max abs error {err:.2e}")
        assert err <= 2e-5, (n, H, Lc, err)
        assert guards_intact(ob, n * Lc * W)
        # row 0 of every sequence is v[0], bit for bit
        v0 = qkv.view(n, Lc, 3 * W)[:, 0, 2 * W:]
        assert torch.equal(bits(got.view(n, Lc, W)[:, 0]), bits(v0)), (n, H, Lc)
        # two runs agree bit for bit
        again = ops.causal_attn_fwd(qkv.to(dev), n, Lc, H).cpu()
        assert torch.equal(bits(again), bits(got))
        # causality, exactly: rows <= t do not see the k and v rows of positions > t
        for t in sorted({0, Lc // 2, Lc - 1}):
            for fill in ("finite", 1e30):
                alt = qkv.clone().view(n, Lc, 3 * W)
                if fill == "finite":
                    alt[:, t + 1:, W:] = torch.randn(n, Lc - t - 1, 2 * W, generator=g) * 3 + 1
                else:
                    alt[:, t + 1:, W:] = fill
                got2 = ops.causal_attn_fwd(alt.view(n * Lc, 3 * W).to(dev), n, Lc, H).cpu().view(n, Lc, W)
                assert torch.equal(bits(got2[:, :t + 1]), bits(got.view(n, Lc, W)[:, :t + 1])), (n, H, Lc, t, fill)
                if fill == "finite" and t < Lc - 1:         # (nothing lies above the last row)
                    assert not torch.equal(got2[:, t + 1:], got.view(n, Lc, W)[:, t + 1:])


def test_causal_attention_refusals(dev):
    from semivl_amd import ops
    L_, lib = _lib()
    qkv, out = torch.zeros(193 * 192, device=dev), torch.zeros(193 * 64, device=dev)
    for (n, Lc, H), word in (((1, 193, 1), "L 193"), ((1, 0, 1), "L 0"), ((1, 8, 0), "H 0"), ((0, 8, 1), "n 0")):
        assert lib.svl_causal_attn_fwd_f32(_p(qkv), n, Lc, H, _p(out), _st()) == -1
        assert "svl_causal_attn_fwd_f32" in L_.last_error() and word in L_.last_error(), L_.last_error()
        with pytest.raises(RuntimeError, match=word):
            ops.causal_attn_fwd(qkv, n, Lc, H)
    assert lib.svl_causal_attn_fwd_f32(None, 1, 8, 1, _p(out), _st()) == -1 and "qkv" in L_.last_error()
    assert lib.svl_causal_attn_fwd_f32(_p(qkv), 1, 8, 1, None, _st()) == -1 and "out" in L_.last_error()
    assert bool((out == 0).all())


# ---- svl_quickgelu_f32 ---------------------------------------------------------------------------------------------------
SPECIALS = [0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 1e4, -1e4, float("inf"), float("-inf"), float("nan")]
BEYOND_ONE_PASS = 2048 * 256 * 4 + 5          # the capped grid's 2048 blocks of 256 threads cover 4 elements each per pass


def _quickgelu_inputs(size, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(size, generator=g) * 3
    k = min(size, len(SPECIALS))
    if size >= len(SPECIALS):
        x[:k] = torch.tensor(SPECIALS)
    else:
        x[:k] = torch.tensor(SPECIALS)[torch.randperm(len(SPECIALS), generator=g)[:k]]
    return x


def _quickgelu_check(x, got):
    """The bound is measured, not chosen: torch's own fp32 evaluation of x * sigmoid(1.702 x) on the host against float64, worst
    relative error over the finite inputs whose float64 result is a normal fp32 number (below that a relative error says
    nothing: fp32 cannot hold the value); the kernel gets 4 x that (another exp) plus 2^-149 absolute."""
    t32 = x * torch.sigmoid(1.702 * x)
    ref = x.double() * torch.sigmoid(1.702 * x.double())
    fin = torch.isfinite(x)
    normal = fin & (ref.abs() >= 2.0 ** -126)
    torch_rel = ((t32.double() - ref).abs() / ref.abs())[normal].max().item() if normal.any() else U
    torch_rel = max(torch_rel, U)                                    # (a lucky draw cannot push the bound under one rounding)
    err = (got.double() - ref).abs()
    bound = 4 * torch_rel * ref.abs() + 2.0 ** -149
    own_rel = (err / ref.abs())[normal].max().item() if normal.any() else 0.0
    assert bool((err[fin] <= bound[fin]).all()), (own_rel, torch_rel, x[fin][(err[fin] > bound[fin])][:5])
    # the edges, pinned to what fp32 torch gives
    pinf, ninf, nan = x == float("inf"), x == float("-inf"), torch.isnan(x)
    assert bool((got[pinf] == float("inf")).all()) and bool((t32[pinf] == float("inf")).all())
    assert bool(torch.isnan(t32[ninf]).all()) and bool(torch.isnan(got[ninf]).all())     # -inf * 0 is NaN in torch: so here
    assert bool(torch.isnan(got[nan]).all())
    big_neg = fin & (x <= -80)
    assert bool((got[big_neg] == 0).all()) and not bool(torch.isnan(got[fin]).any())
    zero = x == 0
    assert torch.equal(bits(got[zero]), bits(t32[zero]))                                   # the sign of zero goes through
    return own_rel, torch_rel


@pytest.mark.parametrize("size", [1, 3, 4, 5, 1023, 1025, BEYOND_ONE_PASS])
def test_quickgelu(dev, size):
    L_, lib = _lib()
    x = _quickgelu_inputs(size, size)
    worst = (0.0, 0.0)
    for off, in_place in itertools.product((0, 1), (False, True)):      # off 1: 4 bytes past a 16-byte boundary
        guard = 64 + off
        xb, xv = guarded(size, dev, guard=guard)
        xv.copy_(x)
        assert xv.data_ptr() % 16 == 4 * off
        if in_place:
            yb, yv = xb, xv
        else:
            yb, yv = guarded(size, dev, guard=guard)
        assert lib.svl_quickgelu_f32(_p(xv), _p(yv), size, _st()) == 0, L_.last_error()
        got = yv.cpu()
        assert guards_intact(yb, size, guard)
        if not in_place:
            assert torch.equal(bits(xv.cpu()), bits(x))
        worst = max(worst, _quickgelu_check(x, got))
    print(f"quickgelu size {size}: kernel worst relative error {worst[0]:.3e}, torch fp32 on the host {worst[1]:.3e}")


def test_quickgelu_wrapper_and_refusals(dev):
    from semivl_amd import ops
    L_, lib = _lib()
    x = _quickgelu_inputs(4099, 9)
    y = ops.quickgelu(x.to(dev))
    _quickgelu_check(x, y.cpu())
    z = x.to(dev)
    assert ops.quickgelu(z, out=z) is z and torch.equal(bits(z.cpu()), bits(y.cpu()))
    assert lib.svl_quickgelu_f32(None, _p(z), 4, _st()) == -1 and "svl_quickgelu_f32: x" in L_.last_error()
    assert lib.svl_quickgelu_f32(_p(z), None, 4, _st()) == -1 and "svl_quickgelu_f32: y" in L_.last_error()
    assert lib.svl_quickgelu_f32(_p(z), _p(z), 0, _st()) == -1 and "count 0" in L_.last_error()


# ---- svl_gather_rows_f32 -------------------------------------------------------------------------------------------------
def test_gather_rows_bit_equal_with_guards(dev):
    L_, lib = _lib()
    g = torch.Generator().manual_seed(4)
    for n, Lc, E in itertools.product((1, 3, 5), (1, 9, 77), (33, 64, 512)):
        x = torch.randn(n * Lc, E, generator=g)
        idx = torch.randint(0, Lc, (n,), generator=g).int()
        idx[0] = Lc - 1
        idx[-1] = 0
        ob, o = guarded(n * E, dev)
        x_d, idx_d = x.to(dev), idx.to(dev)
        assert lib.svl_gather_rows_f32(_p(x_d), _p(idx_d), n, Lc, E, _p(o), _st()) == 0, L_.last_error()
        want = x.view(n, Lc, E)[torch.arange(n), idx.long()]
        assert torch.equal(bits(o.cpu()), bits(want.reshape(-1))), (n, Lc, E)
        assert guards_intact(ob, n * E)
    from semivl_amd import ops
    assert torch.equal(ops.gather_rows(x_d, idx_d, Lc).cpu(), want)
    # an index outside [0, L) reads nothing: its row is NaN, the others are right
    bad = idx.clone()
    bad[0] = Lc
    got = ops.gather_rows(x_d, bad.to(dev), Lc).cpu()
    assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1:], want[1:])
    assert lib.svl_gather_rows_f32(_p(x_d), None, n, Lc, E, _p(o), _st()) == -1
    assert "svl_gather_rows_f32: idx" in L_.last_error()
    assert lib.svl_gather_rows_f32(_p(x_d), _p(idx_d), n, 0, E, _p(o), _st()) == -1 and "L 0" in L_.last_error()


# ---- svl_segment_mean_f32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [33, 512])
def test_segment_mean(dev, E):
    from semivl_amd import ops
    from semivl_amd.model.text_embeddings import class_to_concept_idxs_from_counts, concept_offsets
    counts = [45, 3, 1]
    g = torch.Generator().manual_seed(E)
    x = torch.randn(sum(counts), E, generator=g)
    offs = concept_offsets(class_to_concept_idxs_from_counts(counts), dev)
    assert offs.dtype == torch.int32 and offs.tolist() == [0, 45, 48, 49]
    got = ops.segment_mean(x.to(dev), offs).cpu()
    ref = R.segment_mean(x, counts)
    o = 0
    for c, n in enumerate(counts):
        bound = gamma(n + 1) * x[o:o + n].double().abs().sum(0) / n
        err = (got[c].double() - ref[c]).abs()
        assert bool((err <= bound).all()), (c, (err / bound).max().item())
        o += n
    assert torch.equal(bits(got[2]), bits(x[48]))                       # a segment of one row is a copy
    assert torch.equal(bits(ops.segment_mean(x.to(dev), offs).cpu()), bits(got))
    ones = torch.arange(0, sum(counts) + 1, dtype=torch.int32, device=dev)
    assert torch.equal(bits(ops.segment_mean(x.to(dev), ones).cpu()), bits(x))
    # guard bands, through the library itself
    L_, lib = _lib()
    ob, ov = guarded(3 * E, dev)
    x_d = x.to(dev)
    assert lib.svl_segment_mean_f32(_p(x_d), sum(counts), E, _p(offs), 3, _p(ov), _st()) == 0, L_.last_error()
    assert torch.equal(bits(ov.cpu()), bits(got.reshape(-1))) and guards_intact(ob, 3 * E)


def test_segment_mean_refusals(dev):
    from semivl_amd import ops
    L_, lib = _lib()
    x = torch.randn(6, 8, device=dev)
    for table in ([0, 3, 3, 6], [0, 4, 2, 6], [0, 2, 4], [1, 3, 6], [0]):
        with pytest.raises(ValueError):
            ops.segment_mean(x, torch.tensor(table, dtype=torch.int32, device=dev))
    offs = torch.tensor([0, 6], dtype=torch.int32, device=dev)
    out = torch.zeros(7 * 8, device=dev)
    assert lib.svl_segment_mean_f32(_p(x), 6, 8, _p(offs), 7, _p(out), _st()) == -1     # 7 segments over 6 rows
    assert "svl_segment_mean_f32" in L_.last_error() and "empty" in L_.last_error()
    assert lib.svl_segment_mean_f32(_p(x), 6, 8, None, 1, _p(out), _st()) == -1 and "offsets" in L_.last_error()
    assert lib.svl_segment_mean_f32(None, 6, 8, _p(offs), 1, _p(out), _st()) == -1 and "x is null" in L_.last_error()
    assert bool((out == 0).all())
