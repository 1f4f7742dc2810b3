"""The hand-over path on GENERAL CSC patterns against the exact host model (tests/exact_model.py), bit for bit: k_perturb -> plain f!
(FD_F_SPARSE, the residual the library ships for any pattern) -> k_decompress_list / _sorted / _window / _window2d.  This is the path
that the store routes (tests/test_gpu_storetable.py), the decompression kernels among each other (tests/test_gpu_parity.py), the
device-built plans, the chunked calls, the column windows and the f_in arm are all compared with -- and the path any user's own f!
takes.  Random, rectangular and ragged patterns (empty rows and columns, one dense row), greedy (non-cyclic), partly missing and
invalid colourings, more than kRegColors = 8 colours, the dense-J destination, Float32, and the operand families of
tests/test_gpu_exact_model.py (signed zeros, cancelling rows, step sizes at the edges of the division's range, the scaled norm,
subnormals, NaN / Inf coordinates).  The cases live in tests/exact_general.py (pure numpy: tests/test_exact_model.py evaluates the
model on every one of them on the CPU).  Every case asserts which kernel ran.

Which kernel a forced switch can reach is the plan builder's rule (csrc/fdjac_plan_list.hip), restated in _expected_kernel:
  sorted     needs 4 tiles of 2048 entries (nnz >= 8192), else the plain list kernel runs
  sorted     (the tiny patterns stay below that: there the switch must fall back to the list kernel, and the case asserts that it did)
  window     a tile holds at most kWinMaxCol = 8 consecutive colours: the window kernels take the colourings with at most 6
             colours (their row windows fit the 52 KB of LDS at all three tile sizes); the greedy colourings of random_band (19
             colours) and of the grid (10) cannot reach them
  window2d   the 2-D tiles of the grid pattern, with the grid's own 5 colours or the invalid 6 (its greedy colouring has 10)
  auto       no switch: the device builder (DevicePatternCSC) describes one-window tiles and 2-D tiles only; random_band's tiles are
             neither, and its storage order is a scattered gather, so it builds colour-sorted index lists"""
import numpy as np
import pytest

import exact_general as G
from test_gpu_exact_model import _check
import finitediff_jl_amd as fd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SWITCHES = ("FDJAC_WINDOW", "FDJAC_WINDOW2D", "FDJAC_SORTED", "FDJAC_WIN_TILE", "FDJAC_PLAN_DEVICE")


def _expected_kernel(case, nnz, C):
    """(INFO_WINDOW, INFO_WINDOW2D, INFO_SORTED_GATHER) the case must report."""
    k = case["kernel"]
    if case["variant"] == "dense" or k == "list":
        return 0, 0, 0
    if k == "sorted":
        return 0, 0, int(nnz >= 4 * 2048)
    if k == "auto":                                  # the device builder's index lists for a scattered storage order (random_band)
        return 0, 0, 1
    assert C <= 8, case["id"]                        # (kWinMaxCol: the window kernels' cases use the colourings of at most 6 colours)
    return (1, 0, 0) if k == "window" else (1, 1, 0)


def _set_switches(monkeypatch, case):
    monkeypatch.setenv("FDJAC_SMALL", "0")            # the defined two-level order of the step-size reduction at every N
    monkeypatch.setenv("FDJAC_LAZY_STORE", "0")
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    k = case["kernel"]
    if k == "list":
        monkeypatch.setenv("FDJAC_WINDOW", "0")
        monkeypatch.setenv("FDJAC_SORTED", "0")
    elif k == "sorted":
        monkeypatch.setenv("FDJAC_SORTED", "1")
    elif k == "window":
        monkeypatch.setenv("FDJAC_WINDOW", "1")
        monkeypatch.setenv("FDJAC_WINDOW2D", "0")
        monkeypatch.setenv("FDJAC_SORTED", "0")       # (a colouring the window kernel cannot hold then takes the list kernel)
        if case["tile"]:
            monkeypatch.setenv("FDJAC_WIN_TILE", str(case["tile"]))
    elif k == "window2d":
        monkeypatch.setenv("FDJAC_WINDOW", "1")
        monkeypatch.setenv("FDJAC_WINDOW2D", "1")


@pytest.mark.parametrize("case", G.CASES, ids=[c["id"] for c in G.CASES])
def test_hand_over_path_on_general_patterns(monkeypatch, case):
    _set_switches(monkeypatch, case)
    inp = G.inputs(case)
    M, N, colptr, rowval, colors, C, dtype = (inp[k] for k in ("M", "N", "colptr", "rowval", "colors", "C", "dtype"))
    fdtype, variant = case["fdtype"], case["variant"]
    t = torch.float64 if dtype == np.float64 else torch.float32
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=t, device="cuda")
    kw = {}
    nnz_local = rowval.size
    if variant == "chunked":        # room for two colours' points and values at a time
        rnd = lambda n: (n + 31) // 32 * 32
        kw["scratch_bytes"] = 2 * (2 if fdtype == "central" else 1) * np.dtype(dtype).itemsize * (rnd(N) + rnd(M)) + 4096
    if variant == "colwindow":
        kw["col_window"] = G.COL_WINDOW
        nnz_local = int(colptr[G.COL_WINDOW[1]] - colptr[G.COL_WINDOW[0]])
    if variant == "dense":
        sp = fd.SparseMatrixCSC(M, N, colptr, rowval)
        out = nan(N, M).t()                                          # column-major M x N
        plan = fd.make_plan(out, sp, colors, fdtype, dtype=dtype, **kw)
    elif variant == "device":
        dev = lambda a: torch.as_tensor(a.astype(np.int32), device="cuda")
        out = nan(rowval.size)
        J = fd.DevicePatternCSC(M, N, dev(colptr), dev(rowval), out)
        plan = fd.make_plan(J, J, dev(colors), fdtype, dtype=dtype)
    else:
        J = fd.SparseMatrixCSC(M, N, colptr, rowval)
        plan = fd.make_plan(J, J, colors, fdtype, dtype=dtype, **kw)
        out = nan(plan.out_len(0))
        assert plan.out_len(0) == nnz_local
    f = fd.BuiltinF.sparse(M, N, colptr, rowval, dtype=dtype)
    f_in = None if inp["f_in"] is None else torch.as_tensor(inp["f_in"], device="cuda")
    got = tuple(plan.info(k) for k in (fd.lib.INFO_WINDOW, fd.lib.INFO_WINDOW2D, fd.lib.INFO_SORTED_GATHER))
    flags = dict(kernel=got, nchunks=plan.info(fd.lib.INFO_NCHUNKS), device=plan.info(fd.lib.INFO_BUILT_ON_DEVICE),
                 lazy_store=plan.info(fd.lib.INFO_LAZY_STORE), small=plan.info(fd.lib.INFO_SMALL_FUSED), C=plan.info(fd.lib.INFO_NCOLORS))
    plan.jacobian(f, torch.as_tensor(inp["x"], device="cuda"), [out], f_in=f_in, relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"])
    want = G.layout(case, inp)

    def want_checked(D):
        lay = want(D)
        # the comparison means something only while most of the values are finite (tests/exact_general.py, MIN_FINITE)
        assert lay[0].size == 0 or np.isfinite(lay[0]).mean() >= G.MIN_FINITE, float(np.isfinite(lay[0]).mean())
        return lay
    _check(plan, [out], want_checked, inp["x"], inp["c0"], C, fdtype, inp["rel"], inp["ab"], case["dir"], dtype, inp["f"],
           defined_order=C <= 8, f_in=inp["f_in"])
    # which kernel ran (the plan's choice is fixed at its creation; asserted last so that a wrong kernel still shows its values' verdict)
    assert got == _expected_kernel(case, nnz_local, C), (case["id"], flags)
    assert flags["lazy_store"] == 0 and flags["small"] == 0 and flags["C"] == C, flags
    assert flags["device"] == (1 if variant == "device" else 0), flags
    assert (flags["nchunks"] > 1) if variant == "chunked" else (flags["nchunks"] == (1 if C else 0)), flags
