"""The restarted GMRES of the sparse consumer on the CPU: the numpy model of csrc/fdjac_cscgmres.hip (tests/csc_gmres_model.py) against
a dense solve, the properties GMRES has in exact arithmetic, the case BiCGStab cannot solve, deliberately wrong variants of the model
(which these inputs must expose), and the new symbols at the ABI.

The bound of the dense comparison.  The solve stops at ||b - A y||_2 <= rtol ||b||_2 (the estimate; its own rounding is of the order of
eps and goes into the same factor), so ||y - x||_2 = ||A^-1 (b - A y)||_2 <= ||A^-1|| rtol ||b||_2 <= kappa_2(A) rtol ||x||_2; the dense
solve itself is within kappa_2(A) N eps of x.  Hence ||y - x_dense||_2 / ||x_dense||_2 <= kappa_2(A) (rtol + N eps), kappa_2 by numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as M
import csc_gmres_model as G

try:
    from scipy.linalg import solve as dense_solve
except ImportError:        # pragma: no cover
    dense_solve = np.linalg.solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
RTOL, MAXIT = 1e-10, 400

PATTERNS = {
    "lap5": lambda: M.lap5_pattern(9, 7),
    "tridiag": lambda: M.tridiag_pattern(300),
    "band": lambda: M.random_band_pattern(400, 20, 5, 3),
    "odd": lambda: M.odd_pattern(500, 77, 60, 1),          # one row of 60 entries: the long-row sum
}
_cases = {}


def make_case(name, target=0.9, seed=5):
    """Pattern `name`, values and b in [-1, 1], A = I - gamma J with gamma * max ||row of J||_1 = target; the dense A, its solution and
    its condition number are computed once."""
    key = (name, target, seed)
    if key not in _cases:
        colptr, rowval, N = PATTERNS[name]()
        rng = np.random.default_rng(seed)
        nz = rng.uniform(-1.0, 1.0, rowval.size)
        b = rng.uniform(-1.0, 1.0, N)
        J = np.zeros((N, N))
        J[rowval, np.repeat(np.arange(N), np.diff(colptr))] = nz
        gamma = target / np.abs(J).sum(axis=1).max()
        A = np.eye(N) - gamma * J
        _cases[key] = dict(colptr=colptr, rowval=rowval, N=N, nz=nz, b=b, gamma=float(gamma), rl=M.RowLists(colptr, rowval, N),
                           x=dense_solve(A, b), kappa=float(np.linalg.cond(A)))
    return _cases[key]


def separating_case(k):
    """N = 2 k, one stored entry per 2-block, J[2i, 2i + 1] = 2, alpha = beta = 1: every block of A is [[1, 2], [0, 1]];
    b = (1, -1, 1, -1, ...); the solution is (3, -1, 3, -1, ...).  Returns (colptr, rowval, N, nz, b, x)."""
    N = 2 * k
    colptr = np.zeros(N + 1, dtype=np.int64)
    colptr[2::2] = 1
    colptr = np.cumsum(colptr)
    rowval = np.arange(0, N, 2, dtype=np.int64)
    return colptr, rowval, N, np.full(k, 2.0), np.tile([1.0, -1.0], k), np.tile([3.0, -1.0], k)


def problems(c, restart, fault=None):
    """Every comparison of this file on case c with the model variant `fault`: the list of those that fail."""
    out = []
    tr = {}
    y, st = G.solve(c["rl"], 1.0, -c["gamma"], c["nz"], c["b"], RTOL, MAXIT, restart=restart, fault=fault, trace=tr)
    if st["flags"] != 0 or not np.all(np.isfinite(y)):
        return ["flags %d" % st["flags"]]
    err = np.linalg.norm(y - c["x"]) / np.linalg.norm(c["x"])
    bound = c["kappa"] * (RTOL + c["N"] * EPS)
    if not err <= bound:
        out.append("error %.3e > bound %.3e" % (err, bound))
    for cyc, est in enumerate(tr["est"]):                     # non-increasing within a cycle, up to 4 eps gamma per step
        for a, b in zip(est, est[1:]):
            if not b <= a + 4 * EPS * est[0]:
                out.append("cycle %d: the estimate rises from %.17g to %.17g" % (cyc, a, b))
    for cyc in range(1, len(tr["gammas"])):                   # the explicit gamma of a restart against the estimate before it
        prev = tr["est"][cyc - 1][-1]
        if not abs(tr["gammas"][cyc] - prev) <= 1e-6 * prev:
            out.append("cycle %d: gamma %.17g, the estimate was %.17g" % (cyc, tr["gammas"][cyc], prev))
    V = tr["V"][:tr["len"]]                                   # the last cycle's basis is orthonormal (the bound of the GPU test)
    dev = np.abs(V @ V.T - np.eye(tr["len"])).max()
    if not dev <= 64 * EPS * restart:
        out.append("V^T V - I = %.3e" % dev)
    return out


INPUTS = [(name, restart) for name in PATTERNS for restart in (5, 30)]


@pytest.mark.parametrize("name,restart", INPUTS)
def test_model_against_the_dense_solve_and_the_properties_of_gmres(name, restart):
    c = make_case(name)
    assert problems(c, restart) == []
    y, st = G.solve(c["rl"], 1.0, -c["gamma"], c["nz"], c["b"], RTOL, MAXIT, restart=restart)
    assert st["flags"] == 0 and 1 <= st["iterations"] < MAXIT and st["resid"] <= RTOL * st["bnorm"]
    print("%s restart %d: iterations %d resid %.3e kappa %.2f" % (name, restart, st["iterations"], st["resid"], c["kappa"]))


def test_the_cases_take_more_than_one_cycle_and_have_a_long_row():
    assert make_case("odd")["rl"].nlong == 1
    tr = {}
    G.solve(make_case("lap5")["rl"], 1.0, -make_case("lap5")["gamma"], make_case("lap5")["nz"], make_case("lap5")["b"], RTOL, MAXIT, restart=5, trace=tr)
    assert len(tr["gammas"]) >= 3


@pytest.mark.parametrize("fault", [f for f in G.FAULTS if f])
def test_a_wrong_model_is_exposed_by_these_inputs(fault):
    failing = [(name, restart) for name, restart in INPUTS if problems(make_case(name), restart, fault)]
    print(fault, failing)
    assert failing


@pytest.mark.parametrize("precond", [("jacobi",), ("block", 2), ("block", 32), ("ilu", 64)])
def test_model_with_every_preconditioner(precond):
    c = make_case("lap5")
    y, st = G.solve(c["rl"], 1.0, -c["gamma"], c["nz"], c["b"], RTOL, MAXIT, restart=30, precond=precond)
    assert st["flags"] == 0 and np.linalg.norm(y - c["x"]) / np.linalg.norm(c["x"]) <= c["kappa"] * (RTOL + c["N"] * EPS)


@pytest.mark.parametrize("k", [1, 1025])
def test_the_separating_case_on_both_models(k):
    colptr, rowval, N, nz, b, x = separating_case(k)
    rl = M.RowLists(colptr, rowval, N)
    y, st = M.solve(rl, 1.0, 1.0, nz, b, 1e-10, 500)
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))          # rhat . v = 0 exactly
    for restart in (2, 30):
        y, st = G.solve(rl, 1.0, 1.0, nz, b, 1e-10, 500, restart=restart)
        assert st["flags"] == 0 and st["iterations"] == 2
        assert np.abs(y - x).max() / np.abs(x).max() <= 1e-9


def test_model_edge_cases():
    c = make_case("tridiag")
    rl, N, nz, g = c["rl"], c["N"], c["nz"], c["gamma"]
    y, st = G.solve(rl, 1.0, -g, nz, np.zeros(N))                                     # b = 0
    assert st == {"flags": 0, "iterations": 0, "resid": 0.0, "bnorm": 0.0} and np.array_equal(y, np.zeros(N))
    y, st = G.solve(rl, 1.0, -g, nz, c["b"], RTOL, 7, restart=30)                     # the iterations run out in the middle of a cycle
    assert st["flags"] == 1 and st["iterations"] == 7 and np.all(np.isnan(y))
    yk, stk = G.solve(rl, 1.0, -g, nz, c["b"], RTOL, 7, restart=30, keep_unconverged=True)
    assert stk == st and np.all(np.isfinite(yk)) and np.linalg.norm(yk - c["x"]) < np.linalg.norm(c["x"])
    nzn = nz.copy(); nzn[5] = np.nan
    y, st = G.solve(rl, 1.0, -g, nzn, c["b"])
    assert st["flags"] == 2 and np.all(np.isnan(y))
    nz0 = nz.copy(); nz0[rl.diag[17]] = 1.0 / g                                       # 1 - g / g = 0: a zero diagonal
    y, st = G.solve(rl, 1.0, -g, nz0, c["b"])
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    colptr, rowval, N2, nz2, b2, x2 = separating_case(1)                              # restart > N: the Krylov space is exhausted,
    tr = {}                                                                           # H[2, 1] is zero up to rounding: converged
    y, st = G.solve(M.RowLists(colptr, rowval, N2), 1.0, 1.0, nz2, b2, 1e-10, 500, restart=30, trace=tr)
    assert st["flags"] == 0 and st["iterations"] == 2 and tr["H"][1][2] <= EPS and np.abs(y - x2).max() <= 3e-9
    one = M.RowLists(np.array([0, 1]), np.array([0]), 1)                              # N = 1: v_0 = +-1, so H[1, 0] = 0 EXACTLY and the
    tr = {}                                                                           # cycle ends there: converged, not a breakdown
    y, st = G.solve(one, 1.0, -0.5, np.array([0.5]), np.array([3.0]), 1e-10, 500, restart=5, trace=tr)
    assert st["flags"] == 0 and st["iterations"] == 1 and tr["H"][0][1] == 0.0 and y[0] == 4.0
    b32 = c["b"].astype(np.float32)                                                   # Float32 in and out, Float64 inside
    y32, st = G.solve(rl, 1.0, -g, nz.astype(np.float32), b32, 1e-6, 50)
    y64, _ = G.solve(rl, 1.0, -g, nz.astype(np.float32).astype(np.float64), b32.astype(np.float64), 1e-6, 50)
    assert y32.dtype == np.float32 and st["flags"] == 0 and np.array_equal(y32, y64.astype(np.float32))


def test_abi_declares_exports_and_validates_the_method():
    """Without a device no solver exists, so only the NULL handle can be refused here; the ranges of method and restart are checked on
    a live solver in tests/test_gpu_cscgmres.py."""
    names = ["csc_solver_set_method", "csc_solver_gmres_basis"]
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    fd.lib.build()
    L = fd.lib.load()
    for pre in ("fd_", "fd32_"):
        for n in names:
            assert re.search(r"^int %s%s\(" % (pre, n), hdr, re.M), pre + n
            assert hasattr(L, pre + n) and pre + n in fd.lib.EXPORTS
        assert getattr(L, pre + "csc_solver_set_method")(None, 1, 30) == 1            # FD_ERR_ARG
        assert b"solver is NULL" in L.fd_last_error()
        assert getattr(L, pre + "csc_solver_gmres_basis")(None, None, None, None, None) == 1
    for macro, value in (("FD_CSC_METHOD_BICGSTAB", 0), ("FD_CSC_METHOD_GMRES", 1), ("FD_CSC_GMRES_RESTART_MAX", G.RESTART_MAX)):
        assert re.search(r"^#define %s\s+%d\b" % (macro, value), hdr, re.M), macro
    assert hasattr(fd.CscSolver, "set_method") and hasattr(fd.CscSolver, "gmres_basis")
    shim = open(os.path.join(ROOT, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    for n in names:
        assert '"%s"' % n in shim, n
    assert os.path.exists(os.path.join(ROOT, "examples", "csc_gmres_client.c"))
