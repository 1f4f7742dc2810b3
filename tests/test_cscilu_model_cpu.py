"""The block ILU(0) preconditioner of the sparse consumer on the CPU: the numpy model of k_cs_ilu_factor / k_cs_ilu_apply
(tests/csc_ilu_model.py) against an independent dense masked IKJ loop (bit for bit), against the backward-error bounds of an LU
factorisation, and on the grid cases of the feature's issue against the model's own diagonal solve -- and the new symbols at the ABI.

The bounds (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., theorems 9.3 and 8.5 carried over to a fixed pattern: an
update that is dropped is no rounding error).  With gamma_n = n eps / (1 - n eps), n the block's length:
  on every in-block position  |(L U)_ij - a_ij| <= gamma_n (|L| |U|)_ij;
  on a block whose pattern is closed under elimination the computed z of L U z = x satisfies |L U z - x| <= 2 gamma_n |L| |U| |z|
  (the products on the left in np.longdouble: their own rounding is 2^-11 of the bound's)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as M
import csc_block_model as BM
import csc_ilu_model as IM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
RTOL, MAXIT = 1e-10, 500


# ---- patterns and values ------------------------------------------------------------------------------------------------------------------
def stencil_values(nx, ny, slow, fast):
    """nzval on csc_solve_model.lap5_pattern(nx, ny) of J = T_slow (x) I + I (x) T_fast, T = tridiag[sub, diag, super], x the fastest index."""
    k = np.arange(nx * ny)
    i, j = k % nx, k // nx
    keep = np.stack([j > 0, i > 0, k >= 0, i < nx - 1, j < ny - 1], axis=1)          # rows k - nx, k - 1, k, k + 1, k + nx of column k
    vals = np.broadcast_to(np.array([slow[2], fast[2], slow[1] + fast[1], fast[0], slow[0]], dtype=np.float64), keep.shape)
    return vals[keep]


# the table of the feature's issue, N = 48 x 48 = 2304: (name, slow stencil, fast stencil, gamma), A = I - gamma J
GRID = 48
TABLE = [("lap5_g10", (1.0, -2.0, 1.0), (1.0, -2.0, 1.0), 10.0),
         ("lap5_g100", (1.0, -2.0, 1.0), (1.0, -2.0, 1.0), 100.0),
         ("convdiff_g50", (1.8, -2.0, 0.2), (1.5, -2.0, 0.5), 50.0)]


def grid_case(name, nx=GRID, ny=GRID):
    _, slow, fast, gamma = [t for t in TABLE if t[0] == name][0]
    colptr, rowval, N = M.lap5_pattern(nx, ny)
    b = np.random.default_rng(17).standard_normal(N)
    return colptr, rowval, N, stencil_values(nx, ny, slow, fast), b, gamma


def ragged_pattern(n=300, dense_row=77, dense_col=150, seed=4):
    """csc_solve_model.odd_pattern (empty rows, empty columns, missing diagonals, a dense row of 2 n / 3 entries) with a dense column
    added: every row but the empty ones (r = 1 mod 5)."""
    colptr, rowval, n = M.odd_pattern(n, dense_row, 2 * n // 3, seed)
    cols = [list(rowval[colptr[j]:colptr[j + 1]]) for j in range(n)]
    cols[dense_col] = sorted(set(cols[dense_col]) | {r for r in range(n) if r % 5 != 1})
    colptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    return colptr, np.array([r for c in cols for r in c], dtype=np.int64), n


def ragged_case():
    """-> colptr, rowval, N, nz, b, gamma with gamma * max ||row||_1 = 0.9 but for the rows the dense column's entry dominates."""
    colptr, rowval, N = ragged_pattern()
    rng = np.random.default_rng(21)
    nz = rng.uniform(-1.0, 1.0, rowval.size)
    rl = M.RowLists(colptr, rowval, N)
    norms = np.bincount(rowval, weights=np.abs(nz), minlength=N)
    gamma = 0.9 / np.sort(norms)[-2]                                  # the dense row's norm is the largest: it is not dominant
    assert rl.nlong >= 1 and (rl.diag < 0).any() and (rl.lens == 0).any() and rl.lens.max() > 32
    return colptr, rowval, N, nz, rng.standard_normal(N), float(gamma)


def small_cases():
    """(name, colptr, rowval, N, block sizes) of at most 120 rows: what the dense reference can walk."""
    out = [("tridiag100", *M.tridiag_pattern(100), (2, 7, 64, 100, 1024)), ("lap5_12x9", *M.lap5_pattern(12, 9), (5, 36, 64, 108)),
           ("ragged120", *ragged_pattern(120, 31, 60, 5), (7, 64, 120)), ("dense8x4", *BM.block_tridiag_pattern(4, 8), (8, 16)),
           ("n1", np.array([0, 1]), np.array([0]), 1, (2,)), ("n1_empty", np.array([0, 0]), np.array([], dtype=np.int64), 1, (2,)),
           ("bs_plus_1", *M.tridiag_pattern(8), (7,))]
    return out


def values_for(rowval, seed=3):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, rowval.size)


# ---- the independent reference: a dense masked IKJ loop -------------------------------------------------------------------------------------
def dense_matrix(colptr, rowval, N, alpha, beta, nz):
    """-> (A, S): alpha I + beta J with the library's roundings, and the factor's pattern (the stored entries and the diagonal)."""
    A, S = np.zeros((N, N)), np.zeros((N, N), dtype=bool)
    A[np.arange(N), np.arange(N)] = alpha
    S[np.arange(N), np.arange(N)] = True
    for c in range(N):
        for q in range(colptr[c], colptr[c + 1]):
            r = rowval[q]
            S[r, c] = True
            A[r, c] = np.float64(alpha) + np.float64(beta) * nz[q] if r == c else np.float64(beta) * nz[q]
    return A, S


def dense_ilu0(A, S, bs):
    """IKJ ILU(0) of every diagonal block of A on the pattern S, in place on a copy; entries outside the blocks are left alone."""
    F, N = A.copy(), A.shape[0]
    with np.errstate(all="ignore"):
        for a in range(0, N, bs):
            e = min(a + bs, N)
            for i in range(a, e):
                for k in range(a, i):
                    if not S[i, k]:
                        continue
                    F[i, k] = F[i, k] / F[k, k]
                    for j in range(k + 1, e):
                        if S[k, j] and S[i, j]:
                            F[i, j] = F[i, j] - F[i, k] * F[k, j]
    return F


def _inblock(rl, bs):
    rows = np.repeat(np.arange(rl.N), rl.lens)
    return rows, (rows // bs) == (rl.row_col // bs)


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_factor_equals_a_dense_masked_ikj_loop_bit_for_bit(case):
    name, colptr, rowval, N, sizes = case
    nz = values_for(rowval)
    rl = M.RowLists(colptr, rowval, N)
    for alpha, beta in ((1.0, -0.1), (0.5, 2.0)):
        A, S = dense_matrix(colptr, rowval, N, alpha, beta, nz)
        for bs in sizes:
            sch = IM.Schedule(rl, bs)
            lu, u, bad = IM.factor(sch, alpha, beta, nz)
            F = dense_ilu0(A, S, bs)
            rows, inb = _inblock(rl, bs)
            assert np.array_equal(lu[inb].view(np.uint64), F[rows[inb], rl.row_col[inb]].view(np.uint64)), (name, bs)
            assert np.array_equal(lu[~inb].view(np.uint64), np.zeros((~inb).sum(), dtype=np.uint64))          # +0.0 outside the blocks
            assert np.array_equal(u.view(np.uint64), np.ascontiguousarray(np.diag(F)).view(np.uint64)) and not bad
            # the schedule: the levels by their definition, on the dense pattern
            lev_f, lev_b = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
            for i in range(N):
                ks = [k for k in range(i // bs * bs, i) if S[i, k]]
                lev_f[i] = 1 + max(lev_f[k] for k in ks) if ks else 0
            for i in range(N - 1, -1, -1):
                js = [j for j in range(i + 1, min((i // bs + 1) * bs, N)) if S[i, j]]
                lev_b[i] = 1 + max(lev_b[j] for j in js) if js else 0
            assert np.array_equal(sch.lev_f, lev_f) and np.array_equal(sch.lev_b, lev_b), (name, bs)


@pytest.mark.parametrize("case", small_cases() + [("ragged300", *ragged_pattern(), (64, 256))], ids=lambda c: c[0])
def test_level_order_gives_the_bits_of_row_order_and_the_level_apply_those_of_the_row_apply(case):
    name, colptr, rowval, N, sizes = case
    nz = values_for(rowval, 8)
    rl = M.RowLists(colptr, rowval, N)
    x = np.random.default_rng(2).standard_normal(N)
    for bs in sizes:
        sch = IM.Schedule(rl, bs)
        lu, u, _ = IM.factor(sch, 1.0, -0.1, nz)
        lu2, u2, _ = IM.factor(sch, 1.0, -0.1, nz, order="level")
        assert np.array_equal(lu.view(np.uint64), lu2.view(np.uint64)) and np.array_equal(u.view(np.uint64), u2.view(np.uint64)), (name, bs)
        order = sch.level_order()
        assert np.array_equal(np.sort(order), np.arange(N)) and np.array_equal(order // bs, np.arange(N) // bs)
        z, z2 = IM.apply(sch, lu, u, x), IM.apply_by_rows(sch, lu, u, x)
        assert np.array_equal(z.view(np.uint64), z2.view(np.uint64)), (name, bs)


def _blocks_lu(rl, sch, lu, u, a, e):
    """The dense unit-lower L and upper U of the block [a, e) from the model's arrays."""
    n = e - a
    L, U = np.eye(n), np.zeros((n, n))
    for i in range(a, e):
        for p in range(sch.lo[i], sch.mid[i]):
            L[i - a, rl.row_col[p] - a] = lu[p]
        for p in range(sch.up[i], sch.hi[i]):
            U[i - a, rl.row_col[p] - a] = lu[p]
        U[i - a, i - a] = u[i]
    return L, U


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_factor_meets_the_lu_bound_on_every_in_block_position(case):
    name, colptr, rowval, N, sizes = case
    nz = values_for(rowval, 5)
    rl = M.RowLists(colptr, rowval, N)
    A, S = dense_matrix(colptr, rowval, N, 1.0, -0.1, nz)
    LD = np.longdouble
    worst = 0.0
    for bs in sizes:
        sch = IM.Schedule(rl, bs)
        lu, u, bad = IM.factor(sch, 1.0, -0.1, nz)
        assert not bad
        for a in range(0, N, bs):
            e = min(a + bs, N)
            n = e - a
            L, U = _blocks_lu(rl, sch, lu, u, a, e)
            gam = n * EPS / (1 - n * EPS)
            err = np.abs(L.astype(LD) @ U.astype(LD) - A[a:e, a:e].astype(LD))
            bound = gam * (np.abs(L).astype(LD) @ np.abs(U).astype(LD))
            mask = S[a:e, a:e]
            assert np.all(err[mask] <= bound[mask]), (name, bs, a)
            worst = max(worst, float((err[mask] / np.maximum(bound[mask], LD(1e-300))).max()))
    print("%s: worst |LU - A| / (gamma_n |L||U|) on the pattern = %.3f" % (name, worst))


@pytest.mark.parametrize("case", [c for c in small_cases() if c[0] in ("tridiag100", "dense8x4", "bs_plus_1")], ids=lambda c: c[0])
def test_apply_meets_the_lu_solve_bound_on_closed_patterns(case):
    name, colptr, rowval, N, sizes = case
    nz = values_for(rowval, 6)
    rl = M.RowLists(colptr, rowval, N)
    x = np.random.default_rng(4).standard_normal(N)
    LD = np.longdouble
    for bs in sizes:
        sch = IM.Schedule(rl, bs)
        lu, u, bad = IM.factor(sch, 1.0, -0.1, nz)
        z = IM.apply(sch, lu, u, x)
        for a in range(0, N, bs):
            e = min(a + bs, N)
            n = e - a
            L, U = _blocks_lu(rl, sch, lu, u, a, e)
            gam = n * EPS / (1 - n * EPS)
            lhs = np.abs(L.astype(LD) @ (U.astype(LD) @ z[a:e].astype(LD)) - x[a:e].astype(LD))
            rhs = 2 * gam * (np.abs(L).astype(LD) @ (np.abs(U).astype(LD) @ np.abs(z[a:e]).astype(LD)))
            assert np.all(lhs <= rhs), (name, bs, a)


# ---- the solve on the issue's table ---------------------------------------------------------------------------------------------------------
_JACOBI = {}


def _jacobi(name):
    if name not in _JACOBI:
        colptr, rowval, N, nz, b, gamma = grid_case(name)
        _JACOBI[name] = M.solve(M.RowLists(colptr, rowval, N), 1.0, -gamma, nz, b, RTOL, MAXIT)[1]
    return _JACOBI[name]


@pytest.mark.parametrize("bs", [64, 256, 1024])
@pytest.mark.parametrize("name", [t[0] for t in TABLE])
def test_block_ilu_converges_in_fewer_iterations_than_the_diagonal(name, bs):
    """Observed with the committed models (diagonal | bs = 64, 256, 1024): lap5_g10 61 | 40, 28, 23; lap5_g100 114 | 73, 53, 42;
    convdiff_g50 83 | 36, 17, 14; the true residual at most 0.94 rtol (9.42e-11)."""
    colptr, rowval, N, nz, b, gamma = grid_case(name)
    assert N == 2304
    rl = M.RowLists(colptr, rowval, N)
    sj = _jacobi(name)
    y, st = IM.solve(rl, 1.0, -gamma, nz, b, RTOL, MAXIT, bs=bs)
    res = BM_true_residual(colptr, rowval, nz, N, 1.0, -gamma, y, b)
    print("%s bs %d: diagonal flags %d it %d | block ILU flags %d it %d true residual %.2e" % (name, bs, sj["flags"], sj["iterations"], st["flags"], st["iterations"], res))
    assert sj["flags"] == 0 and st["flags"] == 0
    assert res <= 10 * RTOL
    assert st["iterations"] < sj["iterations"]


def BM_true_residual(colptr, rowval, nz, N, alpha, beta, y, b):
    import test_cscblock_model_cpu as H
    return H.true_residual(colptr, rowval, nz, N, alpha, beta, y, b)


# ---- failure paths --------------------------------------------------------------------------------------------------------------------------
def breakdown_cases():
    """(name, colptr, rowval, N, alpha, beta, nz, b, bs) on the tridiagonal pattern of 100 rows with blocks of 7: a zero first diagonal
    of block 3 with alpha = 0; a NaN in nzval; a pivot that cancels to an exact zero ([[1, 1], [1, 1]] at rows 21, 22)."""
    colptr, rowval, N = M.tridiag_pattern(100)
    rl = M.RowLists(colptr, rowval, N)
    nz = np.random.default_rng(9).uniform(0.5, 1.0, rowval.size)
    b = np.random.default_rng(10).standard_normal(N)
    cols = np.repeat(np.arange(N), np.diff(colptr))
    at = lambda r, c: int(np.nonzero((rowval == r) & (cols == c))[0][0])
    zero = nz.copy(); zero[rl.diag[21]] = 0.0
    nan = nz.copy(); nan[at(40, 41)] = np.nan
    canc = nz.copy()
    canc[rl.diag[21]], canc[rl.diag[22]], canc[at(21, 22)], canc[at(22, 21)] = 0.0, 0.0, -2.0, -2.0          # 1 - 0.5 * 0 = 1 = -0.5 * -2
    return [("zero", colptr, rowval, N, 0.0, 1.0, zero, b, 7), ("nan", colptr, rowval, N, 1.0, -0.1, nan, b, 7),
            ("cancel", colptr, rowval, N, 1.0, -0.5, canc, b, 7)]


def test_a_bad_pivot_is_a_breakdown_with_no_iteration():
    for name, colptr, rowval, N, alpha, beta, nz, b, bs in breakdown_cases():
        rl = M.RowLists(colptr, rowval, N)
        lu, u, bad = IM.factor(IM.Schedule(rl, bs), alpha, beta, nz)
        assert bad, name
        if name == "cancel":
            assert u[21] == 1.0 and u[22] == 0.0
        if name == "zero":
            assert u[21] == 0.0
        y, st = IM.solve(rl, alpha, beta, nz, b, RTOL, MAXIT, bs=bs)
        assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y)), name
        yk, stk = IM.solve(rl, alpha, beta, nz, b, RTOL, MAXIT, keep_unconverged=True, bs=bs)
        assert stk["flags"] == 2 and stk["iterations"] == 0 and np.array_equal(yk, np.zeros(N)), name


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_block_ilu():
    names = ["csc_solver_set_block_ilu", "csc_solver_ilu_levels", "csc_solver_ilu_factors"]
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    assert re.search(r"^#define FD_CSC_ILU_BS_MAX\s+%d\b" % IM.BS_MAX, hdr, re.M)
    assert not re.search(r"^#define FD_CSC_PRECOND_\w+\s+2\b", hdr, re.M)            # no third kind of fd_csc_solver_set_preconditioner
    fd.lib.build()
    L = fd.lib.load()
    shim = open(os.path.join(ROOT, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    for n in names:
        for pre in ("fd_", "fd32_"):
            assert re.search(r"^int %s%s\(" % (pre, n), hdr, re.M), pre + n
            assert hasattr(L, pre + n) and pre + n in fd.lib.EXPORTS
        assert '"%s"' % n in shim, n
    assert "set_block_ilu!(s::CscSolver{$T}, block_size::Integer)" in shim
    for m in ("set_block_ilu", "ilu_levels", "ilu_factors"):
        assert hasattr(fd.CscSolver, m)
    for pre in ("fd_", "fd32_"):                       # argument checks that need no device
        assert getattr(L, pre + "csc_solver_set_block_ilu")(None, 64) == 1                  # FD_ERR_ARG
        assert getattr(L, pre + "csc_solver_ilu_levels")(None, None, None, None, None) == 1
        assert getattr(L, pre + "csc_solver_ilu_factors")(None, None, None, None, None) == 1
        assert getattr(L, pre + "csc_solver_set_preconditioner")(None, 2, 8) == 1


def test_plain_c_client_builds_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = str(tmp_path / "csc_ilu_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    fd.lib.build()
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "csc_ilu_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    if torch.cuda.is_available():
        return                                          # the run itself: tests/test_gpu_cscilu.py
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 7 and "no HIP device" in out.stderr      # FD_ERR_NODEVICE
