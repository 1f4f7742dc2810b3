"""The block-Jacobi preconditioner of the sparse consumer on the CPU: the numpy model of k_cs_binv / k_cs_bapply
(tests/csc_block_model.py) against numpy / SciPy -- the inversion by a bound in the block's own condition number, the gather exactly,
the solve on the reaction-diffusion family against the Jacobi model (tests/csc_solve_model.py), the failure paths -- and the new
symbols at the ABI.

The inversion bound.  Gauss-Jordan with partial pivoting on a block of bs rows is backward stable up to the growth factor: the
computed X satisfies ||X B - I||_inf <= c bs eps kappa_inf(B) with a modest c.  A plain implementation measured at most 0.31 of
bs eps kappa_inf over 560 blocks of the family; the test allows 2."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as M
import csc_block_model as BM

try:
    import scipy.sparse as sp
except ImportError:        # pragma: no cover
    sp = None
needs_scipy = pytest.mark.skipif(sp is None, reason="needs SciPy")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
RTOL, MAXIT = 1e-10, 500
GAMMA = 0.1                      # A = I - 0.1 J

# the table of the feature's issue: (m, nx, ny, k, cond, skew)
TABLE_SYM = [(4, 40, 30, 1e3, 1e3, 0.0), (8, 40, 30, 1e3, 1e3, 0.0), (16, 20, 15, 1e3, 1e3, 0.0), (32, 20, 15, 1e3, 1e3, 0.0)]
TABLE_SKEW = [(4, 40, 30, 1e3, 1e3, 0.3), (8, 40, 30, 1e3, 1e3, 0.3), (16, 20, 15, 1e3, 1e3, 0.3), (32, 20, 15, 1e3, 1e3, 0.3),
              (32, 20, 15, 1e2, 1e2, 1.0)]


def family_case(m, nx, ny, k, cond, skew, seed=3):
    colptr, rowval, nz, N = BM.reaction_diffusion(nx, ny, m, k, cond, skew, seed)
    b = np.random.default_rng(seed + 100).standard_normal(N)
    return colptr, rowval, nz, N, b


def true_residual(colptr, rowval, nz, N, alpha, beta, y, b):
    """||(alpha I + beta J) y - b||_2 / ||b||_2 with every product and sum in np.longdouble."""
    L = np.longdouble
    cols = np.repeat(np.arange(N), np.diff(colptr))
    acc = L(alpha) * np.asarray(y, dtype=L)
    np.add.at(acc, rowval, L(beta) * np.asarray(nz, dtype=L) * np.asarray(y, dtype=L)[cols])
    r = acc - np.asarray(b, dtype=L)
    return float(np.sqrt((r * r).sum()) / np.sqrt((np.asarray(b, dtype=L) ** 2).sum()))


# ---- 1. inversion ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3, 5, 8, 16, 31, 32])
def test_inverse_meets_the_condition_number_bound(m):
    worst = 0.0
    for cond, skew, seed in ((1e1, 0.0, 1), (1e3, 0.3, 2), (1e6, 0.0, 3), (1e6, 1.0, 4)):
        colptr, rowval, nz, N = BM.reaction_diffusion(5, 4, m, cond, cond, skew, seed)
        B = BM.gather_blocks(colptr, rowval, N, 1.0, -GAMMA, nz, m)
        inv, bad = BM.invert_blocks(B)
        assert not bad.any()
        for X, Bk in zip(inv, B):
            err = np.abs(X @ Bk - np.eye(m)).sum(axis=1).max()
            bound = 2 * m * EPS * np.linalg.cond(Bk, np.inf)
            worst = max(worst, err / bound)
            assert err <= bound, (m, cond, skew, err, bound)
    print("m = %d: worst ||X B - I||_inf / (2 bs eps kappa_inf) = %.3f" % (m, worst))


def test_inverse_pivots_by_rows_and_takes_the_lowest_row_on_ties():
    B = np.array([[[0.0, 2.0, 1.0], [1.0, 1.0, 0.0], [-1.0, 0.0, 3.0]]])        # a zero diagonal: needs the swap; |1| = |-1|: row 1 wins
    inv, bad = BM.invert_blocks(B)
    assert not bad.any() and np.abs(inv[0] @ B[0] - np.eye(3)).max() <= 8 * EPS
    # the same elimination by hand with the pivot rows 1, then (of rows 1..2 after the swap) the larger magnitude
    A = np.concatenate([B[0], np.eye(3)], axis=1)
    A[[0, 1]] = A[[1, 0]]
    for j in range(3):
        if j == 1:
            assert abs(A[1, 1]) > abs(A[2, 1])
        piv = A[j, j]
        for i in range(3):
            if i != j:
                A[i] = A[i] - (A[i, j] / piv) * A[j]
        A[j] = A[j] / piv
    assert np.array_equal(inv[0], A[:, 3:])


# ---- 2. gather ---------------------------------------------------------------------------------------------------------------------------
@needs_scipy
@pytest.mark.parametrize("bs", [2, 3, 5, 8, 32])
def test_gather_equals_scipy_slicing(bs):
    colptr, rowval, N = M.odd_pattern(1003, 77, 600, 1)          # empty rows and columns, missing diagonals, a dense row; 1003 = 7 * 11 * 13 + 2
    rl = M.RowLists(colptr, rowval, N)
    assert (rl.diag < 0).any() and (rl.lens == 0).any() and N % bs != 0
    nz = np.random.default_rng(6).uniform(-1, 1, rowval.size)
    alpha, beta = 1.5, -0.25
    J = sp.csc_matrix((nz, rowval, colptr), shape=(N, N)).tocsr()
    stored = sp.csc_matrix((np.ones(rowval.size), rowval, colptr), shape=(N, N)).tocsr()
    for idx, base in ((np.int64, 0), (np.int32, 1), (np.int32, 0), (np.int64, 1)):
        cp, rv = (colptr + base).astype(idx), (rowval + base).astype(idx)        # what the C ABI takes: the model is told the base
        assert cp.dtype == idx and cp[0] == base and rv.min() >= base and rv.max() <= N - 1 + base
        B = BM.gather_blocks(cp, rv, N, alpha, beta, nz, bs, idx_base=base)
        if base:
            planes = BM.block_inverses(cp, rv, N, alpha, beta, nz, bs, idx_base=base)[0]
            assert np.array_equal(planes, BM.block_inverses(colptr, rowval, N, alpha, beta, nz, bs)[0], equal_nan=True)
        empty_row_seen = False
        for k in range((N + bs - 1) // bs):
            a, e = k * bs, min((k + 1) * bs, N)
            Jk, Sk = J[a:e, a:e].toarray(), stored[a:e, a:e].toarray() != 0
            want = np.where(Sk, beta * Jk, 0.0)
            d = np.arange(e - a)
            want[d, d] = np.where(Sk[d, d], alpha + beta * Jk[d, d], alpha)
            assert np.array_equal(B[k, :e - a, :e - a], want), k
            assert not B[k, e - a:, :].any() and not B[k, :, e - a:].any()
            empty_row_seen = empty_row_seen or (~Sk.any(axis=1)).any()
        assert empty_row_seen and (N - (N // bs) * bs) in range(1, bs)


def test_planes_hold_the_columns_of_the_inverses_and_the_apply_multiplies_by_them():
    colptr, rowval, nz, N = BM.reaction_diffusion(3, 3, 5, 10.0, 10.0, 0.3, 2)
    for bs in (5, 4):                                            # 45 = 9 * 5 = 11 * 4 + 1
        planes, bad = BM.block_inverses(colptr, rowval, N, 1.0, -GAMMA, nz, bs)
        B = BM.gather_blocks(colptr, rowval, N, 1.0, -GAMMA, nz, bs)
        x = np.random.default_rng(1).standard_normal(N)
        got = BM.apply_planes(planes, x)
        for k in range((N + bs - 1) // bs):
            a, e = k * bs, min((k + 1) * bs, N)
            inv = BM.invert_blocks(B[k:k + 1, :e - a, :e - a])[0][0]
            assert np.array_equal(planes[:e - a, a:e].T, inv) and not planes[e - a:, a:e].any()
            assert np.abs(got[a:e] - np.linalg.solve(B[k, :e - a, :e - a], x[a:e])).max() <= 1e-12
        assert not bad


# ---- 3. the solve ------------------------------------------------------------------------------------------------------------------------
def _both(case):
    m = case[0]
    colptr, rowval, nz, N, b = family_case(*case)
    rl = M.RowLists(colptr, rowval, N)
    yj, sj = BM.solve(rl, 1.0, -GAMMA, nz, b, RTOL, MAXIT, precond=("jacobi",))
    yb, sb = BM.solve(rl, 1.0, -GAMMA, nz, b, RTOL, MAXIT, precond=("block", m))
    res = true_residual(colptr, rowval, nz, N, 1.0, -GAMMA, yb, b) if sb["flags"] == 0 else float("nan")
    print("m %d cells %dx%d k %g cond %g skew %g: jacobi flags %d it %d | block flags %d it %d true residual %.2e"
          % (case[:6] + (sj["flags"], sj["iterations"], sb["flags"], sb["iterations"], res)))
    return sj, sb, res


@pytest.mark.parametrize("case", TABLE_SYM, ids=lambda c: "m%d" % c[0])
def test_block_jacobi_needs_a_quarter_of_the_iterations(case):
    """Observed with the committed models: Jacobi 78, 83, 77, 77 iterations (m = 4, 8, 16, 32), block Jacobi 6 on every row; the true
    residual of the block solves at most 0.72 rtol (7.11e-11)."""
    sj, sb, res = _both(case)
    assert sj["flags"] == 0 and sb["flags"] == 0
    assert 4 * sb["iterations"] <= sj["iterations"]
    assert res <= 10 * RTOL


@pytest.mark.parametrize("case", TABLE_SKEW, ids=lambda c: "m%d_skew%g" % (c[0], c[5]))
def test_block_jacobi_converges_where_jacobi_fails(case):
    """Observed: the Jacobi model breaks down (flags 2, after 66 .. 173 iterations) on every row; the block model converges in 3 - 4
    iterations with a true residual of at most 0.82 rtol (8.20e-11)."""
    sj, sb, res = _both(case)
    assert sj["flags"] != 0 and sb["flags"] == 0
    assert res <= 10 * RTOL


# ---- 4. failure paths -------------------------------------------------------------------------------------------------------------------
def singular_and_nan_cases():
    """The m = 4 family member with (a) cell 7's block of A made singular: two equal rows; (b) a NaN entry in that block."""
    colptr, rowval, nz, N, b = family_case(4, 12, 10, 1e3, 1e3, 0.0)
    cols = np.repeat(np.arange(N), np.diff(colptr))
    r0, r1 = 7 * 4, 7 * 4 + 1
    sing = nz.copy()
    for c in range(7 * 4, 7 * 4 + 4):                 # rows r0 and r1 of A's block, A = I - 0.1 J, equal BIT FOR BIT: (.., 1, 1, ..)
        q0 = np.nonzero((cols == c) & (rowval == r0))[0][0]
        q1 = np.nonzero((cols == c) & (rowval == r1))[0][0]
        if c == r0:
            sing[q0], sing[q1] = 0.0, -10.0           # 1 - 0.1 * 0 = 1 = -0.1 * -10 (0.1 * 10 rounds to 1)
        elif c == r1:
            sing[q0], sing[q1] = -10.0, 0.0
        else:
            sing[q1] = sing[q0]
    B = BM.gather_blocks(colptr, rowval, N, 1.0, -GAMMA, sing, 4)[7]
    nan = nz.copy()
    nan[np.nonzero((cols == r1) & (rowval == r0))[0][0]] = np.nan
    return colptr, rowval, N, b, sing, nan, B


def test_a_singular_or_nan_block_is_a_breakdown_with_no_iteration():
    colptr, rowval, N, b, sing, nan, B = singular_and_nan_cases()
    rl = M.RowLists(colptr, rowval, N)
    assert np.array_equal(B[0], B[1]) and np.linalg.matrix_rank(B) == 3
    for nz in (sing, nan):
        y, st = BM.solve(rl, 1.0, -GAMMA, nz, b, RTOL, MAXIT, precond=("block", 4))
        assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
        yk, stk = BM.solve(rl, 1.0, -GAMMA, nz, b, RTOL, MAXIT, keep_unconverged=True, precond=("block", 4))
        assert stk["flags"] == 2 and stk["iterations"] == 0 and np.array_equal(yk, np.zeros(N))


@needs_scipy
def test_on_a_dominant_tridiagonal_the_blocks_do_not_cost_iterations():
    import test_cscsolve_model_cpu as H
    colptr, rowval, N, nz, b, gamma, J = H.make_case("tridiag", 0.5)
    assert N == 20000
    rl = M.RowLists(colptr, rowval, N)
    yj, sj = M.solve(rl, 1.0, -gamma, nz, b, RTOL, MAXIT)
    yb, sb = BM.solve(rl, 1.0, -gamma, nz, b, RTOL, MAXIT, precond=("block", 2))
    print("tridiagonal 20000, 0.5: jacobi %d iterations, block 2 %d" % (sj["iterations"], sb["iterations"]))
    assert sj["flags"] == 0 and sb["flags"] == 0 and sb["iterations"] <= sj["iterations"]
    assert true_residual(colptr, rowval, nz, N, 1.0, -gamma, yb, b) <= 10 * RTOL


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_preconditioner():
    names = ["csc_solver_set_preconditioner", "csc_solver_block_inverses"]
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    assert re.search(r"^#define FD_CSC_PRECOND_JACOBI\s+0\b", hdr, re.M) and re.search(r"^#define FD_CSC_PRECOND_BLOCK_JACOBI\s+1\b", hdr, re.M)
    fd.lib.build()
    L = fd.lib.load()
    shim = open(os.path.join(ROOT, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    for n in names:
        for pre in ("fd_", "fd32_"):
            assert re.search(r"^int %s%s\(" % (pre, n), hdr, re.M), pre + n
            assert hasattr(L, pre + n) and pre + n in fd.lib.EXPORTS
        assert '"%s"' % n in shim, n
    assert "set_preconditioner!(s::CscSolver" in shim
    assert hasattr(fd.CscSolver, "set_preconditioner") and hasattr(fd.CscSolver, "block_inverses")
    for pre in ("fd_", "fd32_"):                       # argument checks that need no device
        assert getattr(L, pre + "csc_solver_set_preconditioner")(None, 1, 8) == 1          # FD_ERR_ARG
        assert getattr(L, pre + "csc_solver_block_inverses")(None, None, None, None) == 1
