"""svl_gemm_f32 held to the float64 restatement of its descriptor (tests/gemm_desc_ref.py), one table row per dispatch branch.

Every row is a fixed descriptor (fixed seeds, fixed shapes) launched through ops.gemm in arithmetic mode 0 and mode 6:

* result: |C - C64| <= bound elementwise when an fp32 family served the launch (svl_last_gemm_path() 0, 2, 3; the bound is
  the a-priori bound of a k-ordered fp32 fma chain, derived in gemm_desc_ref.py); on the split families (paths 1, 4) the
  project's own gate: norm-wise error against float64 <= EMU6_ERR_FACTOR x the error of the same descriptor in mode 0;
* nothing else is written: output and preact buffers carry guard rows in front and behind, gap columns and a NaN sentinel
  bit pattern; every element outside the reference's written_mask is bit-identical afterwards, so is every input (whose
  own gaps hold the sentinel too: a loader that reads one poisons the result);
* determinism: a second launch gives the same bits;
* dispatch: the table (tests/gemm_desc_rows.py, shared with the CPU test of the routing) holds the expected
  svl_last_gemm_path() per mode, and the rows together reach every path value; the host-only query svl_gemm_route, asked
  about the same descriptor before each launch, names the path that then ran and the number of operand-maximum passes
  (the svl_absmax_launches() delta around the launch).

K = 0: the argument check accepts it.  Only the exact fp32 kernel can be chosen for it (every other family asks for
K >= 9): its accumulators are zero-initialised, the panel count (kend - kbeg + 15) / 16 is <= 0 so neither the prologue load
nor the k-loop runs, and the epilogue follows unconditionally -- the same holds for an empty split-K range (kend < kbeg),
also in the split kernel (klen <= 0 -> zero steps).  So the rows exist and expect the epilogue of 0.

Set SVL_GEMM_DESC_REPORT=<file> to get the per-row figures (path, worst error / bound or ratio to mode 0, seconds) as JSON.
"""
import ctypes as C
import json
import os
import time

import pytest
import torch

import gemm_desc_ref as R
from gemm_desc_rows import ROWS, bits, cdesc, gemm_args, refusals, route, sentinel

pytestmark = pytest.mark.gpu

EMU6_ERR_FACTOR = 1.2          # the gate of tests/test_ops_gpu.py for every split-product kernel
FP32_PATHS, SPLIT_PATHS = (0, 2, 3), (1, 4)
REPORT = {}


@pytest.fixture
def emu_mode():
    """Switch the arithmetic mode for one test; restore the exact fp32 MFMA and the planes switch afterwards."""
    from semivl_amd import ops

    def use(mode):
        ops.set_gemm_emulation(mode)

    keep = ops.PLANES_PATH
    yield use
    ops.set_gemm_emulation(0)
    ops.PLANES_PATH = keep


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SVL_GEMM_DESC_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------------ the runner
def launch(d, Td, emu_h2):
    """Launches the row; returns (path that ran, the host-only route query of the same descriptor, maximum passes launched)."""
    from semivl_amd import ops
    args, kw = gemm_args(d, Td)
    lib = ops.L.load()
    info = route(d, Td, emu_h2)
    n0 = lib.svl_absmax_launches()
    ops.gemm(*args, emu_h2=emu_h2, **kw)
    torch.cuda.synchronize()
    return lib.svl_last_gemm_path(), info, lib.svl_absmax_launches() - n0


def prepare(d, T):
    """Reference, and the initial buffers: everything the descriptor does not read holds the sentinel."""
    res = R.reference_full(d, T)
    guard = d["ldc_m"] if d["out_mode"] != R.OUT_STRIDED or d["ldc_n"] == 1 else d["ldc_n"]
    outs = [(d["C"], res.written_mask, res.C64, res.bound)]
    if d["preact"] is not None:
        outs.append((d["preact"], res.p_mask, res.P64, res.p_bound))
    for name, mask, _, _ in outs:
        assert not bool(mask[:guard].any()) and not bool(mask[-guard:].any()), "no guard row around the output"
        assert int(mask.sum()) == d["M"] * d["N"] * d["batch"]
        if not (d["accumulate"] and name == d["C"]):
            T[name] = sentinel(T[name].numel()).clone()
        else:
            T[name][~mask] = sentinel(1)
    return outs


def compare(outs, got, path, base):
    """Worst error / bound on an fp32 family; on a split family the norm-wise error and its ratio to mode 0 (`base`)."""
    figures, ok = [], True
    for i, (name, mask, ref, bound) in enumerate(outs):
        g = got[name].double()
        err = (g - ref).abs()[mask]
        nrm = float(err.norm() / ref[mask].norm().clamp_min(1e-300))
        if path in FP32_PATHS:
            b = bound[mask]
            ratio = float(torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf"))).nan_to_num(
                nan=float("inf")).max())
            ok = ok and ratio <= 1.0
            figures.append({"buffer": name, "err_over_bound": ratio, "normwise": nrm})
        else:
            ok = ok and base is not None and nrm <= EMU6_ERR_FACTOR * base[i]["normwise"]
            figures.append({"buffer": name, "normwise": nrm,
                            "ratio_to_mode0": nrm / base[i]["normwise"] if base and base[i]["normwise"] > 0 else float("inf")})
    return figures, ok


@pytest.mark.parametrize("r", ROWS, ids=lambda r: r.name)
def test_descriptor_row(dev, emu_mode, r):
    d, T = r.build()
    inputs = sorted(set(T) - {d["C"], d["preact"]})
    t0 = time.time()
    outs = prepare(d, T)
    t_ref = time.time() - t0
    base, failures = None, []
    for mode in (0, 6):
        emu_mode(mode)
        t0 = time.time()
        Td = {k: v.to(dev) for k, v in T.items()}
        path, info, passes = launch(d, Td, r.emu_h2)
        got = {name: Td[name].cpu() for name, _, _, _ in outs}
        Td2 = {k: (T[k].to(dev) if k in got else v) for k, v in Td.items()}
        path2 = launch(d, Td2, r.emu_h2)[0]
        figures, ok = compare(outs, got, path, base)
        if mode == 0:
            base = figures
        rec = {"path": path, "figures": figures, "seconds": round(time.time() - t0, 3), "reference_seconds": round(t_ref, 3)}
        REPORT.setdefault(r.name, {})[str(mode)] = rec
        print(r.name, "mode", mode, json.dumps(rec))
        if path != r.paths[mode] or path2 != path:
            failures.append(f"mode {mode}: path {path} / {path2}, table says {r.paths[mode]}")
        if info.path != path or info.max_passes != passes:     # the host-only query against the launch it describes
            failures.append(f"mode {mode}: svl_gemm_route says path {info.path}, {info.max_passes} maximum passes; "
                            f"path {path} ran with {passes}")
        if mode == 0 and path not in FP32_PATHS:
            failures.append(f"mode 0 ran on path {path}")
        if not ok:
            failures.append(f"mode {mode}: result outside the gate {figures}")
        for name, mask, _, _ in outs:
            if not torch.equal(bits(got[name])[~mask], bits(T[name])[~mask]):
                bad = (bits(got[name]) != bits(T[name])) & ~mask
                failures.append(f"mode {mode}: {int(bad.sum())} elements of {name} outside the descriptor were written, "
                                f"first at {int(bad.nonzero()[0])}")
            if not torch.equal(bits(Td2[name].cpu()), bits(got[name])):
                failures.append(f"mode {mode}: second launch differs in {name}")
        for k in inputs:
            if not torch.equal(bits(Td[k].cpu()), bits(T[k])):
                failures.append(f"mode {mode}: input {k} was modified")
    assert not failures, failures


def test_rows_reach_every_path_in_each_mode():
    """Mode 0 has the exact kernel, the short-K stream and the elementwise kernel; mode 6 adds both split forms.  Every row
    test asserts that its expected path is the one that ran, so the table's coverage is the launches' coverage."""
    assert {r.paths[0] for r in ROWS} == {0, 2, 3}
    assert {r.paths[6] for r in ROWS} == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what,build,status", refusals(), ids=[r[0].replace(" ", "_") for r in refusals()])
def test_refusal_before_any_launch(dev, emu_mode, what, build, status):
    from semivl_amd import lib as L
    d, T = build()
    for name in {d["C"], d["preact"]} - {None}:
        T[name] = sentinel(T[name].numel()).clone()
    for mode in (0, 6):
        emu_mode(mode)
        Td = {k: v.to(dev) for k, v in T.items()}
        c = cdesc(d, Td)
        rc = L.load().svl_gemm_f32(C.byref(c), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = L.last_error()
        torch.cuda.synchronize()
        assert rc == status and "svl_gemm_f32" in msg, (what, mode, rc, msg)
        assert L.load().svl_gemm_route(C.byref(c), C.byref(L.GemmRouteInfo())) == rc, (what, mode)
        for k in T:
            assert torch.equal(bits(Td[k].cpu()), bits(T[k])), (what, mode, k)
