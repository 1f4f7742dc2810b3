"""The restarted GMRES of the sparse consumer on the device (csrc/fdjac_cscgmres.hip, fd_csc_solver_set_method): y, the flags, the
iteration count, the residual estimate, ||b|| and the basis BIT FOR BIT against the numpy model (tests/csc_gmres_model.py) over one
covering set of sizes, restarts, preconditioners and element types; the ends of a solve (inside a cycle, at a restart, out of
iterations, breakdowns); the case BiCGStab cannot solve; and the switches between the methods on one handle."""
import os
import subprocess

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as M
import csc_block_model as BM
import csc_ilu_model as IM
import csc_gmres_model as G
import test_cscgmres_model_cpu as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
MAXIT = 40          # enough for the well-conditioned cases; the slow ones (restart 1, 2) are compared where they stand


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _solver(colptr, rowval, N, dtype=np.float64):
    return fd.CscSolver((colptr.astype(np.int64), rowval.astype(np.int64), N), dtype=dtype, idx_base=0)


def _select(s, precond):
    if precond[0] == "jacobi":
        s.set_preconditioner("jacobi")
    elif precond[0] == "block":
        s.set_preconditioner("block_jacobi", precond[1])
    else:
        s.set_block_ilu(precond[1])


def _device_solve(s, nz, b, alpha, beta, rtol, maxit=MAXIT, keep=False):
    s.set_options(rtol, maxit)
    s.set_policy(keep)
    y = torch.full((b.size,), 7.0, dtype=_dev(b).dtype, device="cuda")
    s.solve(_dev(nz), _dev(b), y, alpha, beta)
    return y.cpu().numpy(), s.status()


_systems = {}


def system(name):
    """(colptr, rowval, N, nz, b, gamma, RowLists): values and b in [-1, 1], A = I - gamma J with gamma * max ||row of J||_1 = 0.9."""
    if name not in _systems:
        if name == "lap5":
            colptr, rowval, N = M.lap5_pattern(9, 7)
        elif name == "long":
            colptr, rowval, N = M.odd_pattern(1025, 77, 60, 1)          # one row of 60 entries, empty rows and columns
        else:
            colptr, rowval, N = M.tridiag_pattern(int(name))
        rng = np.random.default_rng(N)
        nz = rng.uniform(-1.0, 1.0, rowval.size)
        b = rng.uniform(-1.0, 1.0, N)
        rl = M.RowLists(colptr, rowval, N)
        rows = np.zeros(N)
        np.add.at(rows, rowval, np.abs(nz))
        _systems[name] = (colptr, rowval, N, nz, b, float(0.9 / rows.max()), rl)
    return _systems[name]


# ---- 1. the covering set -----------------------------------------------------------------------------------------------------------------
SIZES = ("1", "2", "255", "1024", "1025", "3079")
RESTARTS = (1, 2, 5, 30, 64)
PRECONDS = (("jacobi",), ("block", 2), ("block", 32), ("ilu", 64))
COVER = []
for _i, _n in enumerate(SIZES):
    for _k, _pc in enumerate(PRECONDS):
        COVER.append((_n, RESTARTS[(4 * _i + _k) % 5], _pc, np.float32 if (_i + _k) % 3 == 0 else np.float64))
for _k, _pc in enumerate(PRECONDS):
    COVER.append(("long", (5, 30, 64, 2)[_k], _pc, np.float32 if _k == 1 else np.float64))
for _r, _pc, _t in ((5, ("jacobi",), np.float64), (5, ("block", 2), np.float32), (30, ("ilu", 64), np.float64), (64, ("block", 32), np.float64),
                    (1, ("jacobi",), np.float32), (2, ("ilu", 64), np.float32)):
    COVER.append(("lap5", _r, _pc, _t))


def test_the_covering_set_covers():
    assert 30 <= len(COVER) <= 45
    assert {c[0] for c in COVER} == set(SIZES) | {"long", "lap5"} and {c[1] for c in COVER} == set(RESTARTS)
    assert {c[2] for c in COVER} == set(PRECONDS) and {c[3] for c in COVER} == {np.float32, np.float64}
    assert system("long")[6].nlong == 1


@pytest.mark.parametrize("case", COVER, ids=lambda c: "%s-m%d-%s-%s" % (c[0], c[1], "".join(map(str, c[2])), np.dtype(c[3]).name))
def test_solve_equals_the_model_bit_for_bit(case):
    name, restart, precond, dtype = case
    colptr, rowval, N, nz, b, gamma, rl = system(name)
    nzt, bt = nz.astype(dtype), b.astype(dtype)
    rtol = 1e-10 if dtype == np.float64 else 1e-6
    want, wst = G.solve(rl, 1.0, -gamma, nzt, bt, rtol, MAXIT, keep_unconverged=True, restart=restart, precond=precond)
    s = _solver(colptr, rowval, N, dtype)
    _select(s, precond)
    s.set_method("gmres", restart)
    got, st = _device_solve(s, nzt, bt, 1.0, -gamma, rtol, keep=True)
    print(case[0], restart, precond, np.dtype(dtype).name, st, wst)
    assert wst["flags"] in (0, 1) and wst["iterations"] >= 1
    assert st == wst
    assert _same_bits(got, want)
    again, st2 = _device_solve(s, nzt, bt, 1.0, -gamma, rtol, keep=True)          # the same bits on every call
    assert st2 == st and _same_bits(again, got)


# ---- 2. the ends of a solve --------------------------------------------------------------------------------------------------------------
def _both(name, restart, rtol=1e-10, maxit=400, keep=False, precond=("jacobi",), nz=None, b=None, trace=None):
    colptr, rowval, N, nz0, b0, gamma, rl = system(name)
    nz, b = nz0 if nz is None else nz, b0 if b is None else b
    want, wst = G.solve(rl, 1.0, -gamma, nz, b, rtol, maxit, keep_unconverged=keep, restart=restart, precond=precond, trace=trace)
    s = _solver(colptr, rowval, N)
    _select(s, precond)
    s.set_method("gmres", restart)
    got, st = _device_solve(s, nz, b, 1.0, -gamma, rtol, maxit, keep)
    return s, got, st, want, wst


def test_convergence_inside_a_cycle_and_exactly_at_a_restart():
    s, got, st, want, wst = _both("255", 64)
    its = wst["iterations"]
    assert wst["flags"] == 0 and 2 < its < 64 and st == wst and _same_bits(got, want)          # inside the first cycle
    tr = {}
    s, got, st, want, wst = _both("255", its, trace=tr)                                        # the cycle's last column converges
    assert wst["flags"] == 0 and wst["iterations"] == its and len(tr["gammas"]) == 1 and st == wst and _same_bits(got, want)
    tr = {}
    s, got, st, want, wst = _both("255", its - 1, trace=tr)                                    # one column short: a second cycle
    assert wst["flags"] == 0 and len(tr["gammas"]) == 2 and st == wst and _same_bits(got, want)


def test_at_least_three_cycles():
    tr = {}
    s, got, st, want, wst = _both("lap5", 5, trace=tr)
    assert wst["flags"] == 0 and len(tr["gammas"]) >= 3 and st == wst and _same_bits(got, want)


def test_the_iterations_run_out_inside_a_cycle():
    for maxit in (7, 13):                                                                      # the first batch; the second
        s, got, st, want, wst = _both("1025", 30, maxit=maxit)
        assert wst["flags"] == 1 and wst["iterations"] == maxit and st == wst and np.all(np.isnan(got)) and np.all(np.isnan(want))
        s, got, st, want, wst = _both("1025", 30, maxit=maxit, keep=True)
        assert wst["flags"] == 1 and st == wst and np.all(np.isfinite(got)) and _same_bits(got, want)


def test_every_batch_size_gives_the_same_bits(monkeypatch):
    for name, restart in (("lap5", 5), ("255", 30)):
        colptr, rowval, N, nz, b, gamma, rl = system(name)
        want, wst = G.solve(rl, 1.0, -gamma, nz, b, 1e-10, 400, restart=restart)
        for batch in ("1", "3", "8", "64"):
            monkeypatch.setenv("FDJAC_CSC_BATCH", batch)
            s = _solver(colptr, rowval, N)
            s.set_method("gmres", restart)
            got, st = _device_solve(s, nz, b, 1.0, -gamma, 1e-10, 400)
            assert st == wst and _same_bits(got, want), (name, batch)


def test_b_zero_and_a_restart_beyond_n():
    s, got, st, want, wst = _both("255", 30, b=np.zeros(255))
    assert st == wst == {"flags": 0, "iterations": 0, "resid": 0.0, "bnorm": 0.0} and np.array_equal(got, np.zeros(255))
    s, got, st, want, wst = _both("2", 30)                      # the Krylov space is exhausted after two columns: converged, no breakdown
    assert wst["flags"] == 0 and wst["iterations"] == 2 and st == wst and _same_bits(got, want)
    tr = {}
    s, got, st, want, wst = _both("1", 5, trace=tr)             # N = 1: H[1, 0] is an exact zero, the cycle ends there, converged
    assert tr["H"][0][1] == 0.0 and wst["flags"] == 0 and wst["iterations"] == 1 and st == wst and _same_bits(got, want)
    assert s.gmres_basis()[1][0, 1].item() == 0.0


def test_breakdowns_are_arithmetic():
    colptr, rowval, N, nz, b, gamma, rl = system("255")
    nzn = nz.copy(); nzn[5] = np.nan
    for precond in PRECONDS:
        s, got, st, want, wst = _both("255", 30, nz=nzn, precond=precond)
        assert wst["flags"] == 2 and st["flags"] == 2 and st["iterations"] == wst["iterations"] and np.all(np.isnan(got)), precond
    nz0 = nz.copy(); nz0[rl.diag[17]] = 1.0 / gamma             # a zero diagonal under the diagonal preconditioner
    s, got, st, want, wst = _both("255", 30, nz=nz0)
    assert st == wst and st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(got))
    s, got, st, want, wst = _both("255", 30, nz=nz0, keep=True)
    assert st == wst and st["flags"] == 2 and np.array_equal(got, np.zeros(N))
    got, st = _device_solve(s, nz, b, 1.0, -gamma, 1e-10, 400)  # the same solver is clean again on regular values
    want, wst = G.solve(rl, 1.0, -gamma, nz, b, 1e-10, 400, restart=30)
    assert st == wst and st["flags"] == 0 and _same_bits(got, want)


# ---- 3. the basis ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,restart,precond", [("1025", 30, ("jacobi",)), ("lap5", 5, ("block", 2)), ("long", 64, ("ilu", 64))])
def test_the_basis_is_orthonormal_and_equals_the_model(name, restart, precond):
    tr = {}
    s, got, st, want, wst = _both(name, restart, precond=precond, trace=tr)
    assert st == wst and st["flags"] == 0
    V, Hd, k = s.gmres_basis()
    V, Hd = V.cpu().numpy(), Hd.cpu().numpy()
    assert k == tr["len"] >= 1 and V.shape == (restart + 1, system(name)[2]) and Hd.shape == (restart, restart + 1)
    dev = np.abs(V[:k] @ V[:k].T - np.eye(k)).max()
    print(name, restart, precond, "columns", k, "V^T V - I", dev)
    assert dev <= 64 * EPS * restart
    assert _same_bits(V[:k], tr["V"][:k]) and _same_bits(Hd[:k], tr["H"][:k])


# ---- 4. the separating case ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 1025])
def test_gmres_solves_what_bicgstab_refuses(k):
    colptr, rowval, N, nz, b, x = H.separating_case(k)
    rl = M.RowLists(colptr, rowval, N)
    s = _solver(colptr, rowval, N)
    got, st = _device_solve(s, nz, b, 1.0, 1.0, 1e-10, 500)
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(got))                # rhat . v = 0 exactly
    for restart in (2, 30):
        s.set_method("gmres", restart)
        got, st = _device_solve(s, nz, b, 1.0, 1.0, 1e-10, 500)
        want, wst = G.solve(rl, 1.0, 1.0, nz, b, 1e-10, 500, restart=restart)
        assert st == wst and st["flags"] == 0 and st["iterations"] == 2 and _same_bits(got, want)
        assert np.abs(got - x).max() / np.abs(x).max() <= 1e-9


# ---- 5. switching ------------------------------------------------------------------------------------------------------------------------
def test_switching_the_method_leaves_nothing_behind():
    colptr, rowval, N, nz, b, gamma, rl = system("1025")
    args = (nz, b, 1.0, -gamma, 1e-10, 400)
    fresh_j, fst_j = _device_solve(_solver(colptr, rowval, N), *args)                          # BiCGStab-only handles
    fb = _solver(colptr, rowval, N)
    fb.set_preconditioner("block_jacobi", 8)
    fresh_b, fst_b = _device_solve(fb, *args)
    assert fst_j == M.solve(rl, 1.0, -gamma, nz, b, 1e-10, 400)[1] and fst_j["flags"] == 0
    s = _solver(colptr, rowval, N)
    s.set_method("gmres", 30)
    g1, gst1 = _device_solve(s, *args)
    want, wst = G.solve(rl, 1.0, -gamma, nz, b, 1e-10, 400, restart=30)
    assert gst1 == wst and gst1["flags"] == 0 and _same_bits(g1, want)
    s.set_method("bicgstab")
    again, ast = _device_solve(s, *args)
    assert ast == fst_j and _same_bits(again, fresh_j)
    s.set_method("gmres", 5)                                                                   # a smaller restart in the same buffers
    s.set_preconditioner("block_jacobi", 8)
    g2, gst2 = _device_solve(s, *args)
    want2, wst2 = G.solve(rl, 1.0, -gamma, nz, b, 1e-10, 400, restart=5, precond=("block", 8))
    assert gst2 == wst2 and gst2["flags"] == 0 and _same_bits(g2, want2) and s.gmres_basis()[0].shape[0] == 6
    s.set_method("bicgstab")
    again, ast = _device_solve(s, *args)
    assert ast == fst_b and _same_bits(again, fresh_b)
    s.set_preconditioner("jacobi")
    s.set_method("gmres", 64)                                                                  # a larger one: the buffers grow
    g3, gst3 = _device_solve(s, *args)
    want3, wst3 = G.solve(rl, 1.0, -gamma, nz, b, 1e-10, 400, restart=64)
    assert gst3 == wst3 and _same_bits(g3, want3)


# ---- 6. bad arguments --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_errors():
    colptr, rowval, N = M.tridiag_pattern(100)
    for dtype in (np.float64, np.float32):
        s = _solver(colptr, rowval, N, dtype)
        for method, restart in ((2, 30), (-1, 30), (1, 0), (1, -1), (1, 65)):
            assert s.Lt.fd_csc_solver_set_method(s.handle, method, restart) == 1, (method, restart)        # FD_ERR_ARG
        assert s.Lt.fd_csc_solver_set_method(s.handle, 0, -5) == 0                                         # BiCGStab ignores restart
        assert s.Lt.fd_csc_solver_set_method(s.handle, 1, 1) == 0 and s.Lt.fd_csc_solver_set_method(s.handle, 1, 64) == 0
        with pytest.raises(fd.lib.FdError) as e:
            s.gmres_basis()                                                                                # no GMRES solve yet
        assert e.value.code == 3
        with pytest.raises(ValueError):
            s.set_method("cg")


# ---- 7. the C client ---------------------------------------------------------------------------------------------------------------------
def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "csc_gmres_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "csc_gmres_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "csc gmres: bicgstab: status 2 iterations 0" in out.stdout and "csc gmres: gmres(30): status 0 iterations 2" in out.stdout, out.stdout
    assert "csc gmres: PASS" in out.stdout, out.stdout
