"""CPU: the routing of svl_gemm_f32 is host arithmetic on a descriptor, so it is held to its table without a GPU.

* svl_gemm_route on every row of tests/gemm_desc_rows.py, in arithmetic modes 0 and 6 (svl_set_gemm_emulation is host
  state), reports the path the table expects -- the same table tests/test_gemm_desc_gpu.py holds the launches to; it reports
  operand-maximum passes only for the fp16 x 2 form, a ragged split only for the ragged row, and the refusals' statuses.
* the split-K planner (ops._ksplit_plan), which now asks the library for the tile shape and the residency, returns the plan
  of the parent's planner, kept here verbatim as the restatement (its own copies of the tile shapes, of the
  M >= 256 / N >= 96 threshold, of the weight-gradient rule and of the 768 / 512 resident blocks).
"""
import ctypes as C
import math

import pytest

from gemm_desc_rows import ROWS, cdesc, refusals, route


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as g
    g.build()


@pytest.fixture
def emu_mode():
    from semivl_amd import ops
    yield ops.set_gemm_emulation
    ops.set_gemm_emulation(0)


@pytest.mark.parametrize("r", ROWS, ids=lambda r: r.name)
def test_route_of_descriptor_row(emu_mode, r):
    d, T = r.build()
    for mode in (0, 6):
        emu_mode(mode)
        info = route(d, T, r.emu_h2)
        assert info.path == r.paths[mode], (mode, info.path)
        if d["conv"] is None:      # (with a convolution, path 4 is also the whole-image dilated kernel's)
            assert info.h2 == (info.path == 4), (mode, info.h2)
        if info.path != 4:
            assert info.max_passes == 0, (mode, info.max_passes)
        assert info.ragged_rows == (8200 % 128 if r.name == "ragged_fork_M8200" else 0), (mode, info.ragged_rows)


@pytest.mark.parametrize("what,build,status", refusals(), ids=[r[0].replace(" ", "_") for r in refusals()])
def test_query_refuses_what_the_launch_refuses(emu_mode, what, build, status):
    from semivl_amd import lib as L
    d, T = build()
    for mode in (0, 6):
        emu_mode(mode)
        info = L.GemmRouteInfo()
        assert L.load().svl_gemm_route(C.byref(cdesc(d, T)), C.byref(info)) == status, (what, mode, L.last_error())


# ------------------------------------------------------------------------------------------------------ the planner
def parent_ksplit_plan(M, N, K, dense=False, emu_tiles=False):
    """ops._ksplit_plan of the parent commit, verbatim."""
    from semivl_amd.ops import get_gemm_emulation
    bm = 32 if M <= 32 else (64 if M <= 64 else 128)
    bn = 128 if (M <= 64 and N > 64) else (32 if N <= 32 else (64 if N <= 64 else 128))
    tiles = math.ceil(M / bm) * math.ceil(N / bn)
    slots = 768
    if emu_tiles or (dense and M >= 256 and N >= 96 and get_gemm_emulation()):
        tiles, slots = math.ceil(M / 128) * math.ceil(N / 128), 512   # the emulated kernel keeps 2 blocks per CU
    # slices so that tiles x slices fills, but does not exceed, ONE round of resident blocks (256 CUs x 3): 36 tiles x 29
    # slices = 1044 blocks was 1.36 rounds, i.e. a second, mostly idle round
    s = max(1, min(slots // tiles if tiles <= slots else 1, K // 512 if K >= 1024 else 1, 512))
    ks = math.ceil(math.ceil(K / s) / 16) * 16
    s = math.ceil(K / ks)
    return s, ks


def parent_conv_wgrad_plan(Co, N, Kpix, Wo):
    """The planner rule of the parent's ops.conv_wgrad / ops.convT2x_wgrad, verbatim."""
    from semivl_amd.ops import get_gemm_emulation
    x6 = (get_gemm_emulation() in (3, 6) and Co >= 96 and N >= 96 and Wo % 8 == 0 and Kpix >= 1024 and Kpix % 16 == 0)
    return parent_ksplit_plan(Co, N, Kpix, emu_tiles=x6)


SIZES = (20, 50, 64, 96, 128, 256, 300, 768, 2304, 3072)
DEPTHS = (257, 1024, 32800, 16 * 32800)


@pytest.mark.parametrize("mode", (0, 3, 6))
def test_dense_plan_equals_the_parents(emu_mode, mode):
    from semivl_amd import ops
    emu_mode(mode)
    for M in SIZES:
        for N in SIZES:
            for K in DEPTHS:
                assert ops._ksplit_plan(ops.A_MC, ops.B_NC, M, N, K, M, N) == parent_ksplit_plan(M, N, K, dense=True), (M, N, K)


def conv_wgrad_cases():
    """(Co, N, Kpix, lda, ldb, geom): the aligned weight-gradient rows of the table, then the layer kinds of the VOC head (3x3,
    dilated 3x3, 1x1, two sources, the k 2 / s 2 form of the transposed convolutions) over Co x Wo."""
    for r in ROWS:
        d, _ = r.build() if r.name.startswith(("conv_wgrad_", "wgrad6_", "big_conv_wgrad")) else (None, None)
        if d is None:
            continue
        cv, A, B = d["conv"], d["A"], d["B"]
        if any(v % 4 for v in (A["off"], A["ld"], B["off"], B["ld"], cv["C1"], cv["C2"], cv["ld2"], cv["src2_off"])):
            continue
        yield (d["M"], d["N"], d["K"], A["ld"], B["ld"], (cv["H"], cv["W"], cv["C1"], cv["KH"], cv["KW"], cv["dil"], cv["pad"],
                                                          cv["sign"], cv["C2"], cv["rep"], cv["ld2"], cv["stride"], cv["Ho"], cv["Wo"]))
    for Co in (32, 64, 96, 128, 256):
        for Wo in (24, 28, 32, 128):
            for imgs, H, C1, k, dil, C2, rep in ((2, 24, 16, 3, 1, 0, 1), (16, 32, 128, 3, 6, 0, 1), (16, Wo, 256, 1, 1, 0, 1),
                                                 (21, Wo, 32, 3, 1, 64, 21)):
                pad = dil * (k // 2)
                yield Co, k * k * (C1 + C2), imgs * H * Wo, Co, C1, (H, Wo, C1, k, k, dil, pad, 1, C2, rep, C2, 1, H, Wo)
            yield Co, 4 * 32, 4 * 64 * Wo, Co, 32, (128, 2 * Wo, 32, 2, 2, 1, 0, 1, 0, 1, 0, 2, 64, Wo)


@pytest.mark.parametrize("mode", (0, 3, 6))
def test_conv_wgrad_plan_equals_the_parents(emu_mode, mode):
    from semivl_amd import ops
    emu_mode(mode)
    cases = list(conv_wgrad_cases())
    assert len(cases) >= 100
    for Co, N, Kpix, lda, ldb, geom in cases:
        Wo = geom[-1] or geom[1]
        assert ops._ksplit_plan(ops.A_MC, ops.B_CONVW, Co, N, Kpix, lda, ldb, True, geom) == parent_conv_wgrad_plan(Co, N, Kpix, Wo), \
            (Co, N, Kpix, geom)


def test_plan_follows_the_kernel_on_unaligned_operands(emu_mode):
    """The one place the parent's guess and the library could disagree: an im2col weight gradient whose operands cannot
    take 16-byte loads stays on the exact kernel (gemm.hip), so its plan is the exact kernel's -- 128-row tiles, three
    blocks per CU -- where the parent planned for the split kernel.  The product passes no such operands."""
    from semivl_amd import ops
    emu_mode(6)
    geom = (32, 32, 128, 3, 3, 6, 6, 1, 0, 1, 0, 1, 32, 32)
    args = (ops.A_MC, ops.B_CONVW, 128, 9 * 128, 64 * 1024, 128, 128)
    split, exact = parent_ksplit_plan(128, 9 * 128, 64 * 1024, emu_tiles=True), parent_ksplit_plan(128, 9 * 128, 64 * 1024)
    assert split != exact
    assert ops._ksplit_plan(*args, True, geom) == split
    assert ops._ksplit_plan(*args, False, geom) == exact
