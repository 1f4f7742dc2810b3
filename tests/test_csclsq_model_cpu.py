"""The least-squares consumer on the CPU: the numpy model of csrc/fdjac_csclsq.hip (tests/csc_lsq_model.py) against SciPy -- the lists,
both products, the accuracy of the preconditioned CGLS recurrence by a DERIVED bound, its failure paths -- and the new symbols at the ABI.

The bound.  A = J^T J + mu W is symmetric positive definite with smallest eigenvalue lambda_min, and s(y) = J^T (b - J y) - mu W y is
A (y* - y) for the exact minimiser y*.  For any two vectors y, z:  y - z = A^-1 (s(z) - s(y)), hence
    ||y - y_ref||_2 <= (||s(y)||_2 + ||s(y_ref)||_2) / lambda_min,
with s evaluated in np.longdouble.  So that the bound cannot hide a failure its right-hand side must itself be at most
1e-6 ||y_ref||_2, the project's relative contract.

The products.  Each result is a sum of n rounded products in SOME order; whatever the order, |computed - exact| <= (n + 1) eps sum|terms|
to first order (n - 1 additions and one multiplication per term).  Model and SciPy each stay within that, so they differ by at most
2 (n + 2) eps sum|terms|, n = the longest row / column; the final rounding to the output's type is within the + 2."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_lsq_model as LM

try:                       # SciPy is the reference of every test below but the ABI test, which must run without it
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
except ImportError:        # pragma: no cover
    sp = spla = None
needs_scipy = pytest.mark.skipif(sp is None, reason="needs SciPy")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, MAXIT = 1e-10, 500
CASES = {"big": LM.BAND_BIG, "padded": LM.BAND_PADDED}
_cache = {}


def band_case(name, dtype=np.float64):
    """(colptr, rowval, nz, M, N, b, lists) of a rect_band case, built once."""
    key = (name, np.dtype(dtype).name)
    if key not in _cache:
        colptr, rowval, nz, M, N = LM.rect_band(**CASES[name])
        b = np.random.default_rng(1).uniform(-1.0, 1.0, M)
        _cache[key] = (colptr, rowval, nz.astype(dtype), M, N, b.astype(dtype), LM.RectLists(colptr, rowval, M, N))
    return _cache[key]


def model_solution(name, mu, kind, dtype=np.float64):
    key = ("solve", name, mu, kind, np.dtype(dtype).name)
    if key not in _cache:
        colptr, rowval, nz, M, N, b, rl = band_case(name, dtype)
        _cache[key] = LM.solve(rl, mu, kind, nz, b, RTOL, MAXIT)
    return _cache[key]


def reference(name, mu, kind):
    """(J, W, lambda_min, y_ref) by a sparse direct solve of the normal equations, built once per case."""
    key = ("ref", name, mu, kind)
    if key not in _cache:
        colptr, rowval, nz, M, N, b, rl = band_case(name)
        J = sp.csc_matrix((nz, rowval, colptr), shape=(M, N))
        g = np.asarray(J.multiply(J).sum(axis=0)).ravel()
        W = g if kind == LM.DAMP_COLNORM else np.ones(N)
        A = (J.T @ J + mu * sp.diags(W)).tocsc()
        lmin = float(spla.eigsh(A, k=1, sigma=0, which="LM", return_eigenvectors=False)[0])
        _cache[key] = (J, W, lmin, spla.spsolve(A, J.T @ b))
    return _cache[key]


def derived_bound(name, mu, kind, y):
    """(error, bound, bound / ||y_ref||) of the module docstring for the vector y."""
    colptr, rowval, nz, M, N, b, rl = band_case(name)
    J, W, lmin, y_ref = reference(name, mu, kind)
    coo = J.tocoo()
    data, bl, Wl = coo.data.astype(np.longdouble), b.astype(np.longdouble), W.astype(np.longdouble)

    def grad_norm(v):
        v = np.asarray(v, dtype=np.longdouble)
        Jv = np.zeros(M, dtype=np.longdouble)
        np.add.at(Jv, coo.row, data * v[coo.col])
        s = np.zeros(N, dtype=np.longdouble)
        np.add.at(s, coo.col, data * (bl - Jv)[coo.row])
        s = s - np.longdouble(mu) * Wl * v
        return np.sqrt((s * s).sum())

    assert lmin > 0
    err = np.linalg.norm(np.asarray(y, dtype=np.float64) - y_ref)
    bound = float((grad_norm(y) + grad_norm(y_ref)) / lmin)
    return err, bound, bound / np.linalg.norm(y_ref)


@needs_scipy
def test_lists_equal_a_host_counting_sort():
    pats = [LM.rect_band(**LM.BAND_PADDED), LM.rect_band(700, 40, 5, 3), LM.rect_odd()]
    for colptr, rowval, nz, M, N in pats:
        rl = LM.RectLists(colptr, rowval, M, N)
        slots = sp.csc_matrix((np.arange(1, rowval.size + 1, dtype=np.float64), rowval, colptr), shape=(M, N)).tocsr()
        slots.sort_indices()
        assert np.array_equal(rl.row_ptr, slots.indptr) and np.array_equal(rl.row_col, slots.indices)
        assert np.array_equal(rl.row_slot, slots.data.astype(np.int64) - 1)
        assert np.array_equal(rl.long_cols, [j for j in range(N) if colptr[j + 1] - colptr[j] > 32])
        assert rl.nlong == sum(1 for r in range(M) if slots.indptr[r + 1] - slots.indptr[r] > 32)
    rl = LM.RectLists(*[LM.rect_band(**LM.BAND_PADDED)[i] for i in (0, 1, 3, 4)])
    assert list(rl.long_cols) == [7, 1500, 2999] and rl.col_lens[100] == 32
    big = band_case("big")[6]
    assert big.nlong > 0 and big.lens.max() > 100 and big.long_cols.size == 0      # (the clipped ends: rows of ~125 entries)
    colptr, rowval, nz, M, N = LM.rect_odd()
    rl = LM.RectLists(colptr, rowval, M, N)
    assert M < N and rl.nlong == 1 and rl.lens.max() > 256 and (rl.lens == 0).any() and (rl.col_lens == 0).any()


@needs_scipy
@pytest.mark.parametrize("pat", ["padded", "small", "odd"])
def test_products_equal_scipy_to_the_derived_bound(pat):
    colptr, rowval, nz, M, N = {"padded": lambda: LM.rect_band(**LM.BAND_PADDED), "small": lambda: LM.rect_band(701, 40, 5, 3),
                                "odd": LM.rect_odd}[pat]()
    rl = LM.RectLists(colptr, rowval, M, N)
    rng = np.random.default_rng(9)
    J = sp.csc_matrix((nz, rowval, colptr), shape=(M, N))
    eps = np.finfo(float).eps
    for T, transpose, n_in, longest in ((J, False, N, rl.lens.max()), (J.T, True, M, rl.col_lens.max())):
        v = rng.uniform(-1, 1, n_in)
        got = LM.matvec(rl, nz, v, transpose)
        mag = abs(T) @ np.abs(v)
        assert got.shape == (T.shape[0],)
        assert np.all(np.abs(got - T @ v) <= 2 * (int(longest) + 2) * eps * mag)
    g = LM.col_norms(rl, nz)
    g_ref = np.asarray(J.multiply(J).sum(axis=0)).ravel()
    assert np.all(np.abs(g - g_ref) <= 2 * (int(rl.col_lens.max()) + 2) * eps * g_ref)


@needs_scipy
@pytest.mark.parametrize("mu,kind", LM.MU_W)
@pytest.mark.parametrize("name", ["big", "padded"])
def test_model_solve_meets_the_derived_bound(name, mu, kind):
    colptr, rowval, nz, M, N, b, rl = band_case(name)
    y, r, st = model_solution(name, mu, kind)
    print("%s mu %g kind %d: iterations %d grad %.3e grad0 %.3e" % (name, mu, kind, st["iterations"], st["grad"], st["grad0"]))
    assert st["flags"] == 0 and 1 <= st["iterations"] < MAXIT and st["grad"] <= RTOL * st["grad0"]
    err, bound, rel = derived_bound(name, mu, kind, y)
    print("    error %.3e bound %.3e = %.3e ||y_ref||" % (err, bound, rel))
    assert rel <= 1e-6
    assert err <= bound
    # the recurred residual is b - J y to rounding
    J = reference(name, mu, kind)[0]
    assert np.linalg.norm(r - (b - J @ y)) <= 1e-12 * np.linalg.norm(b)


def test_model_failure_paths_and_edge_cases():
    colptr, rowval, nz, M, N = LM.rect_odd()
    rl = LM.RectLists(colptr, rowval, M, N)
    b = np.random.default_rng(2).uniform(-1, 1, M)
    # an empty column that nothing damps: m_j = 0
    y, r, st = LM.solve(rl, 0.0, LM.DAMP_IDENTITY, nz, b)
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y)) and np.all(np.isnan(r))
    y, r, st = LM.solve(rl, 0.5, LM.DAMP_COLNORM, nz, b)                       # W = diag(g): g_j = 0 damps nothing either
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    yk, rk, stk = LM.solve(rl, 0.0, LM.DAMP_IDENTITY, nz, b, keep_unconverged=True)
    assert stk["flags"] == 2 and np.array_equal(yk, np.zeros(N)) and np.array_equal(rk, b)
    # Levenberg's damping reaches the empty columns
    y, r, st = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nz, b)
    assert st["flags"] == 0 and 1 <= st["iterations"] < 500 and st["grad"] <= 1e-10 * st["grad0"]
    assert np.all(y[rl.col_lens == 0] == 0.0)
    # the iterations run out
    y3, r3, st3 = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nz, b, max_iterations=3)
    assert st3["flags"] == 1 and st3["iterations"] == 3 and np.all(np.isnan(y3)) and np.all(np.isnan(r3))
    y3k, r3k, st3k = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nz, b, max_iterations=3, keep_unconverged=True)
    assert st3k == st3 and np.all(np.isfinite(y3k)) and np.all(np.isfinite(r3k))
    # b supported on the empty rows: J^T b = 0 bit for bit, no iteration
    b0 = np.where(rl.lens == 0, b, 0.0)
    assert np.any(b0 != 0)
    y, r, st = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nz, b0)
    assert st == {"flags": 0, "iterations": 0, "grad": 0.0, "grad0": 0.0} and np.array_equal(y, np.zeros(N)) and np.array_equal(r, b0)
    # a NaN in J is a breakdown, not a hang
    nzn = nz.copy(); nzn[5] = np.nan
    y, r, st = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nzn, b)
    assert st["flags"] == 2 and np.all(np.isnan(y))
    # 1 x 1 and Float32 in and out, Float64 inside
    one = LM.RectLists(np.array([0, 1]), np.array([0]), 1, 1)
    y, r, st = LM.solve(one, 0.0, LM.DAMP_IDENTITY, np.array([2.0]), np.array([3.0]))
    assert st["flags"] == 0 and st["iterations"] == 1 and y[0] == 1.5 and r[0] == 0.0
    b32 = b.astype(np.float32)
    y32, r32, st = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nz.astype(np.float32), b32, 1e-6, 100)
    y64, r64, _ = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nz.astype(np.float32).astype(np.float64), b32.astype(np.float64), 1e-6, 100)
    assert y32.dtype == np.float32 and st["flags"] == 0 and np.array_equal(y32, y64.astype(np.float32)) and np.array_equal(r32, r64.astype(np.float32))


def test_abi_declares_and_exports_the_least_squares_consumer():
    names = ["csc_lsq_create", "csc_lsq_destroy", "csc_lsq_matvec_async", "csc_lsq_set_options", "csc_lsq_set_policy",
             "csc_lsq_solve_async", "csc_lsq_status", "csc_lsq_row_lists", "csc_lsq_long_columns"]
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    fd.lib.build()
    L = fd.lib.load()
    for pre in ("fd_", "fd32_"):
        for n in names:
            assert re.search(r"^int %s%s\(" % (pre, n), hdr, re.M), pre + n
            assert hasattr(L, pre + n) and pre + n in fd.lib.EXPORTS
    assert re.search(r"#define FD_CSC_LSQ_DAMP_IDENTITY\s+0\b", hdr) and re.search(r"#define FD_CSC_LSQ_DAMP_COLNORM\s+1\b", hdr)
    assert hasattr(fd, "CscLeastSquares")
    shim = open(os.path.join(ROOT, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    for n in names:
        assert '"%s"' % n in shim, n
    import torch
    if torch.cuda.is_available():
        return                                  # (the GPU tests create consumers)
    colptr, rowval = np.array([0, 1, 2], dtype=np.int64), np.array([0, 2], dtype=np.int64)
    for pre in ("fd_", "fd32_"):
        h = C.c_void_p()
        rc = getattr(L, pre + "csc_lsq_create")(None, 3, 2, colptr.ctypes.data, rowval.ctypes.data, 8, 0, 0, C.byref(h))
        assert rc == 7 and b"no HIP device" in L.fd_last_error()          # FD_ERR_NODEVICE
