"""The sparse consumer on the CPU: the numpy model of csrc/fdjac_cscsolve.hip (tests/csc_solve_model.py) against SciPy -- row lists,
products, the accuracy of the BiCGStab recurrence by a DERIVED bound, its failure paths -- and the new symbols at the ABI.

The bound.  A = I - gamma J strictly row-dominant, delta = min_i(|a_ii| - sum_{j != i} |a_ij|) > 0, so ||A^-1||_inf <= 1 / delta (Varah).
For any two vectors y, z:  y - z = A^-1 ((A y - b) - (A z - b)), hence
    ||y - y_LU||_inf <= (||A y - b||_inf + ||A y_LU - b||_inf) / delta,
with both residuals evaluated in np.longdouble (their own rounding, ~1e-19 relative, is far below either residual)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as M

try:                       # SciPy is the reference of every test below but the ABI test, which must run without it
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
except ImportError:        # pragma: no cover
    sp = spla = None
needs_scipy = pytest.mark.skipif(sp is None, reason="needs SciPy")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, MAXIT = 1e-12, 60          # the model needs 3 .. 21 iterations on the nine dominant cases

PATTERNS = {
    "lap5": lambda: M.lap5_pattern(300, 200),
    "band": lambda: M.random_band_pattern(30000, 300, 6, 11),
    "tridiag": lambda: M.tridiag_pattern(20000),
}


def make_case(name, target, seed=5, dtype=np.float64):
    """Pattern `name` with values in [-1, 1], b in [-1, 1] and gamma such that gamma * max ||row||_1 = target."""
    colptr, rowval, N = PATTERNS[name]()
    rng = np.random.default_rng(seed)
    nz = rng.uniform(-1.0, 1.0, rowval.size).astype(dtype)
    b = rng.uniform(-1.0, 1.0, N).astype(dtype)
    J = sp.csc_matrix((nz.astype(np.float64), rowval, colptr), shape=(N, N))
    gamma = target / abs(J).sum(axis=1).max()
    return colptr, rowval, N, nz, b, float(gamma), J


def derived_bound_holds(J, gamma, b, y):
    """The assertion of the module docstring; returns (error, bound, delta)."""
    N = J.shape[0]
    A = (sp.identity(N, format="csc") - gamma * J).tocsc()
    Ar = A.tocsr()
    diag = np.abs(A.diagonal())
    delta = (diag - (np.asarray(abs(Ar).sum(axis=1)).ravel() - diag)).min()
    assert delta > 0
    y_lu = spla.splu(A).solve(np.asarray(b, dtype=np.float64))
    coo = A.tocoo()

    def resid(z):
        acc = np.zeros(N, dtype=np.longdouble)
        np.add.at(acc, coo.row, coo.data.astype(np.longdouble) * np.asarray(z, dtype=np.longdouble)[coo.col])
        return np.abs(acc - np.asarray(b, dtype=np.longdouble)).max()

    err = np.abs(np.asarray(y, dtype=np.float64) - y_lu).max()
    bound = float((resid(y) + resid(y_lu)) / delta)
    return err, bound, delta


@needs_scipy
def test_row_lists_equal_scipy_csr():
    for colptr, rowval, N in (M.lap5_pattern(13, 9), M.tridiag_pattern(50), M.random_band_pattern(700, 40, 5, 3), M.odd_pattern(4000, 77, 3000, 1)):
        rl = M.RowLists(colptr, rowval, N)
        slots = sp.csc_matrix((np.arange(1, rowval.size + 1, dtype=np.float64), rowval, colptr), shape=(N, N)).tocsr()
        slots.sort_indices()
        assert np.array_equal(rl.row_ptr, slots.indptr) and np.array_equal(rl.row_col, slots.indices)
        assert np.array_equal(rl.row_slot, slots.data.astype(np.int64) - 1)
        cols = np.repeat(np.arange(N), np.diff(colptr))
        want = np.full(N, -1)
        want[cols[rowval == cols]] = np.nonzero(rowval == cols)[0]
        assert np.array_equal(rl.diag, want)
    assert M.RowLists(*M.odd_pattern(4000, 77, 3000, 1)).nlong == 1


@needs_scipy
@pytest.mark.parametrize("pat", [lambda: M.lap5_pattern(40, 30), lambda: M.random_band_pattern(5000, 300, 6, 2), lambda: M.odd_pattern(4000, 77, 3000, 1)])
def test_products_equal_scipy_to_a_few_ulp(pat):
    colptr, rowval, N = pat()
    rng = np.random.default_rng(9)
    nz, v = rng.uniform(-1, 1, rowval.size), rng.uniform(-1, 1, N)
    rl = M.RowLists(colptr, rowval, N)
    A = sp.csc_matrix((nz, rowval, colptr), shape=(N, N))
    scale = abs(A) @ np.abs(v)
    for alpha, beta in ((0.0, 1.0), (1.0, -0.3), (2.5, 0.0)):
        for T, fn in ((A, M.matvec), (A.T, M.matvec_t)):
            want = alpha * v + beta * (T @ v)
            mag = abs(alpha) * np.abs(v) + abs(beta) * (abs(T) @ np.abs(v))
            got = fn(rl, alpha, beta, nz, v)
            assert np.all(np.abs(got - want) <= 16 * np.finfo(float).eps * mag + 1e-300), (alpha, beta)
    assert scale.max() > 0


@needs_scipy
@pytest.mark.parametrize("target", [0.5, 0.9, 0.99])
@pytest.mark.parametrize("name", ["lap5", "band", "tridiag"])
def test_model_solve_meets_the_derived_bound(name, target):
    colptr, rowval, N, nz, b, gamma, J = make_case(name, target)
    rl = M.RowLists(colptr, rowval, N)
    y, st = M.solve(rl, 1.0, -gamma, nz, b, RTOL, MAXIT)
    print("%s %.2f: iterations %d resid %.3e" % (name, target, st["iterations"], st["resid"]))
    assert st["flags"] == 0 and 1 <= st["iterations"] < MAXIT and st["resid"] <= RTOL * st["bnorm"]
    err, bound, delta = derived_bound_holds(J, gamma, b, y)
    print("    error %.3e bound %.3e delta %.3e" % (err, bound, delta))
    assert err <= bound


@needs_scipy
@pytest.mark.parametrize("name", ["lap5", "tridiag"])
def test_model_failure_is_loud(name):
    colptr, rowval, N, nz, b, gamma, J = make_case(name, 3.0)
    rl = M.RowLists(colptr, rowval, N)
    y, st = M.solve(rl, 1.0, -gamma, nz, b, RTOL, 500)
    assert st["flags"] in (1, 2) and np.all(np.isnan(y))
    assert (st["flags"] == 1) == (st["iterations"] == 500)
    yk, stk = M.solve(rl, 1.0, -gamma, nz, b, RTOL, 500, keep_unconverged=True)
    assert stk["flags"] == st["flags"] and stk["iterations"] == st["iterations"] and np.all(np.isfinite(yk))
    y1, st1 = M.solve(rl, 1.0, -gamma, nz, b, RTOL, 1)
    assert st1["flags"] == 1 and st1["iterations"] == 1 and np.all(np.isnan(y1))


@needs_scipy
def test_model_solves_the_non_dominant_band():
    colptr, rowval, N, nz, b, gamma, J = make_case("band", 3.0)
    rl = M.RowLists(colptr, rowval, N)
    y, st = M.solve(rl, 1.0, -gamma, nz, b, RTOL, 500)
    assert st["flags"] == 0 and st["iterations"] < 500
    A = (sp.identity(N, format="csc") - gamma * J).tocsc()
    assert np.abs(A @ y - b).max() <= 1e-9 * np.abs(b).max()


@needs_scipy
def test_model_edge_cases():
    colptr, rowval, N = M.tridiag_pattern(300)
    rl = M.RowLists(colptr, rowval, N)
    nz = np.random.default_rng(1).uniform(-1, 1, rowval.size)
    y, st = M.solve(rl, 1.0, -0.1, nz, np.zeros(N))                     # b = 0
    assert st == {"flags": 0, "iterations": 0, "resid": 0.0, "bnorm": 0.0} and np.array_equal(y, np.zeros(N))
    nz0 = nz.copy()
    nz0[rl.diag[17]] = 4.0                                              # 1 - 0.25 * 4 = 0: a zero Jacobi diagonal
    y, st = M.solve(rl, 1.0, -0.25, nz0, np.ones(N))
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    nzn = nz.copy(); nzn[5] = np.nan
    y, st = M.solve(rl, 1.0, -0.1, nzn, np.ones(N))
    assert st["flags"] == 2 and np.all(np.isnan(y))
    one = M.RowLists(np.array([0, 1]), np.array([0]), 1)                # N = 1
    y, st = M.solve(one, 1.0, -0.5, np.array([0.5]), np.array([3.0]))
    assert st["flags"] == 0 and st["iterations"] == 1 and y[0] == 4.0
    empty = M.RowLists(np.array([0, 0]), np.array([], dtype=np.int64), 1)
    y, st = M.solve(empty, 2.0, -0.5, np.array([]), np.array([3.0]))
    assert st["flags"] == 0 and y[0] == 1.5
    # Float32 in and out, Float64 inside
    b32 = np.random.default_rng(2).uniform(-1, 1, N).astype(np.float32)
    y32, st = M.solve(rl, 1.0, -0.2, nz.astype(np.float32), b32, 1e-6, 50)
    y64, _ = M.solve(rl, 1.0, -0.2, nz.astype(np.float32).astype(np.float64), b32.astype(np.float64), 1e-6, 50)
    assert y32.dtype == np.float32 and st["flags"] == 0 and np.array_equal(y32, y64.astype(np.float32))


def test_abi_declares_and_exports_the_sparse_consumer():
    names = ["csc_solver_create", "csc_solver_destroy", "csc_matvec_async", "csc_solver_set_options", "csc_solver_set_policy",
             "csc_solve_async", "csc_solver_status", "csc_solver_row_lists"]
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    fd.lib.build()
    L = fd.lib.load()
    for pre in ("fd_", "fd32_"):
        for n in names:
            assert re.search(r"^int %s%s\(" % (pre, n), hdr, re.M), pre + n
            assert hasattr(L, pre + n) and pre + n in fd.lib.EXPORTS
    assert hasattr(fd, "CscSolver")
    shim = open(os.path.join(ROOT, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    for n in names:
        assert '"%s"' % n in shim, n
    import torch
    if torch.cuda.is_available():
        return                                  # (the GPU tests create solvers)
    colptr, rowval, N = M.tridiag_pattern(10)
    for pre in ("fd_", "fd32_"):
        h = C.c_void_p()
        rc = getattr(L, pre + "csc_solver_create")(None, N, colptr.ctypes.data, rowval.ctypes.data, 8, 0, 0, C.byref(h))
        assert rc == 7 and b"no HIP device" in L.fd_last_error()          # FD_ERR_NODEVICE
