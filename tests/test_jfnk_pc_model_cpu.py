"""CPU checks of the model of the matrix-free consumer preconditioned by a lagged stored Jacobian (tests/jfnk_pc_model.py, the cases of
tests/jfnk_pc_cases.py): the model composes what exists and equals jfnk_model.solve(d=...) bit for bit where its apply is a division; its
deliberately wrong variants are seen; the case table covers what it says; the stored values equal jfnk_model.jacobian_dense; the
preconditioner pays on the model (what tests/test_gpu_jfnk_pc.py then asks of the device); and the four entry points are declared,
exported and check their arguments before anything else."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as M
import jfnk_cases as JK
import jfnk_model as JM
import jfnk_pc_cases as PC
import jfnk_pc_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- does it help: the setting the GPU test repeats ----------------------------------------------------------------------------------
# tridiag_nl, N = 1000, ONE block of ILU(0) (1024 rows): on a tridiagonal pattern ILU(0) is the exact LU of the lagged matrix.
# I - gamma J(x) stays definite only while gamma * (the largest Gershgorin bound of J, about +1.9 through the nonlinear terms) < 1, so
# gamma was scanned on the model over 0.3 .. 0.8 (central differences, rtol 1e-8, restart 30): the unpreconditioned / preconditioned
# steps were 15 / 5, 19 / 5, 23 / 6, 28 / 6, 35 / 7, 50 / 8.  HELP_GAMMA = 0.7 is the first with a ratio of at least 5; both end with
# flags 0 and true residuals of 7.8e-9 and 4.2e-9 (profiles/jfnk_precond.md).
HELP = dict(family="tridiag_nl", prm=(1000,), fdtype="central", gamma=0.7, rtol=1e-8, restart=30, maxit=500, kind=("ilu", 1024), seed=2024,
            steps_without=35, steps_with=7)


def help_system():
    """(f, x0, x1, b, RowLists, colptr, rowval, nz0): factor at x0, solve at x1 = x0 + 0.05 u."""
    f, x0, b, _d = JK.system(HELP["family"], HELP["prm"])
    N = x0.size
    x1 = x0 + PC.LAG * np.random.default_rng(HELP["seed"]).random(N)
    colptr, rowval, _n = PC.pattern(HELP["family"], HELP["prm"])
    return f, x0, x1, b, M.RowLists(colptr, rowval, N), colptr, rowval, PC.jacobian_nz(HELP["family"], HELP["prm"], x0, colptr, rowval)


def help_models(num_cus=256):
    """((y, status) without a preconditioner, (y, status, trace) with the lagged ILU), at x1."""
    f, _x0, x1, b, rl, _cp, _rv, nz0 = help_system()
    g = HELP["gamma"]
    plain = JM.solve(f, x1, b, 1.0, -g, HELP["fdtype"], None, HELP["rtol"], HELP["maxit"], True, HELP["restart"], num_cus)
    tr = {}
    y, st = PM.solve(f, x1, b, 1.0, -g, rl, (1.0, -g, nz0), HELP["kind"], HELP["fdtype"], HELP["rtol"], HELP["maxit"], True, HELP["restart"],
                     num_cus, trace=tr)
    return plain, (y, st, tr)


@pytest.fixture(scope="module", autouse=True)
def _the_library_has_the_entry_points():
    """The model describes fd_jfnk_solver_set_csc_preconditioner on fd_csc_solver_factor_async: every test here fails on a tree
    without them (one build, shared with the ABI test below)."""
    fd.lib.build()
    L = fd.lib.load()
    assert hasattr(L, "fd_jfnk_solver_set_csc_preconditioner") and hasattr(L, "fd_csc_solver_factor_async")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def test_the_cases_cover():
    sizes = lambda cs: {JK.size_of(c["family"], c["prm"]) for c in cs}          # noqa: E731
    assert set(PC.EDGE_SIZES + PC.SWITCH_SIZES) <= sizes(PC.CASES)
    assert {c["restart"] for c in PC.CASES} == set(PC.RESTARTS)
    assert {c["kind"] for c in PC.CASES} == set(PC.KINDS)
    for fam in ("tridiag", "tridiag_nl", "lap5", "lap5_nl"):          # every kind, both arms, f_in and every route on EACH family
        mine = [c for c in PC.CASES if c["family"] == fam]
        assert {c["kind"][0] for c in mine} == {"jacobi", "block", "ilu"}, fam
        assert {c["fdtype"] for c in mine} == {"forward", "central"}, fam
        assert {bool(c["fin"]) for c in mine if c["fdtype"] == "forward"} == {False, True}, fam
        assert {c["route"] for c in mine} == {"plain", "lazy", "quot"}, fam
        assert {bool(c["xoff"]) for c in mine} == {False, True}, fam
    # the kSmallN switch: block Jacobi 32 and 5 on every route, x on a pair and off it; the fused kernel's tail on both variants
    sw = [c for c in PC.CASES if JK.size_of(c["family"], c["prm"]) in PC.SWITCH_SIZES]
    assert all(c["kind"][0] == "block" for c in sw)
    assert {(c["kind"][1], c["route"]) for c in sw} >= {(bs, r) for bs in (32, 5) for r in ("plain", "lazy", "quot")}
    odd_big = [c for c in sw if JK.size_of(c["family"], c["prm"]) == 16385]
    assert {(c["kind"][1], bool(c["xoff"])) for c in odd_big} == {(bs, o) for bs in (32, 5) for o in (False, True)}
    # the fused kernel at small sizes
    so = [c for c in PC.CASES if c["small_off"]]
    assert sizes(so) == set(PC.SMALL_OFF_SIZES) and {c["kind"] for c in so} == {("block", 2), ("block", 5), ("block", 32)}
    for n in (257, 1025):
        assert {c["kind"][1] for c in so if c["prm"] == (n,)} == {2, 5, 32}
    # the 5-point families: ILU 1024 and block 32 on every grid
    for fam in ("lap5", "lap5_nl"):
        for grid in PC.LAP5_GRIDS:
            assert {c["kind"] for c in PC.CASES if c["family"] == fam and c["prm"] == grid} >= {("ilu", 1024), ("block", 32)}, (fam, grid)
    assert 45 <= len(PC.CASES) <= 62


@pytest.mark.parametrize("family,prm", [("tridiag", (9,)), ("tridiag_nl", (65,)), ("lap5", (4, 5)), ("lap5_nl", (7, 9)), ("lap5_nl", (4, 5))])
def test_the_stored_values_are_jacobian_denses(family, prm):
    colptr, rowval, N = PC.pattern(family, prm)
    x = np.random.default_rng(N).random(N) - 0.25
    D = JM.jacobian_dense(family, prm, x)
    S = np.zeros_like(D)
    S[rowval, np.repeat(np.arange(N), np.diff(colptr))] = PC.jacobian_nz(family, prm, x, colptr, rowval)
    assert _same(S, D)          # the same entries, and nothing of J outside the pattern


@pytest.mark.parametrize("case", [c for c in PC.CASES if JK.size_of(c["family"], c["prm"]) <= 2049][::3], ids=lambda c: c["id"])
def test_with_a_division_as_its_apply_the_model_is_jfnk_models(case):
    """kind ("jacobi",) on the lagged values against jfnk_model.solve(d = the modelled diagonal): y, status, basis, applications."""
    _cp, _rv, rl, _x0, nz0 = PC.stored(case["family"], case["prm"])
    d = np.where(rl.diag >= 0, 1.0 + (-PC.GAMMA0) * nz0[np.maximum(rl.diag, 0)], 1.0)
    f, x, b, _d = JK.system(case["family"], case["prm"])
    fin = f(x) if case["fin"] and case["fdtype"] == "forward" else None
    t0, t1 = {}, {}
    want, wst = JM.solve(f, x, b, 1.0, -PC.GAMMA, case["fdtype"], d, case["rtol"], case["maxit"], True, case["restart"], 256, f_in=fin,
                         x_aligned=not case["xoff"], small_off=case["small_off"], trace=t0)
    got, st = PC.model(case, trace=t1, kind=("jacobi",))
    assert st == wst and _same(got, want) and t0["len"] == t1["len"] and _same(t0["V"], t1["V"]) and _same(t0["H"], t1["H"])
    assert t0["applications"] == t1["applications"]


def test_the_faults_are_seen():
    """Each deliberately wrong variant changes y or the iteration count in at least one case."""
    small = [c for c in PC.CASES if JK.size_of(c["family"], c["prm"]) <= 2049]
    for fault in PM.FAULTS[1:]:
        pool = [c for c in small if c["kind"][0] == "block"] if fault == "fma_apply" else small
        seen = 0
        for c in pool:
            y, st = PC.model(c)
            yf, stf = PC.model(c, fault=fault)
            seen += (st["iterations"] != stf["iterations"]) or not _same(y, yf)
        print(fault, seen, "of", len(pool))
        assert seen >= 1, fault
    # the lag itself: a linear family's J does not depend on x, so "factor_at_x1" shows there through GAMMA0 != GAMMA alone
    lin = next(c for c in small if c["family"] == "tridiag" and c["kind"][0] == "ilu" and c["prm"][0] > 2)
    assert not _same(PC.model(lin)[0], PC.model(lin, fault="factor_at_x1")[0])


def test_a_bad_pivot_of_the_factorisation_ends_the_solve_at_once():
    case = next(c for c in PC.CASES if c["prm"] == (65,))
    _cp, _rv, rl, _x0, nz0 = PC.stored(case["family"], case["prm"])
    nz = nz0.copy()
    nz[rl.diag[4]] = 1.0 / PC.GAMMA0                          # 1 - GAMMA0 * J_44: a zero diagonal ...
    y, st = PC.model(case, keep=False, lagged=(1.0, -PC.GAMMA0, nz), kind=("jacobi",))
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    y, st = PC.model(case, keep=True, lagged=(1.0, -PC.GAMMA0, nz), kind=("jacobi",))
    assert st["flags"] == 2 and np.array_equal(y, np.zeros(65))


def test_the_lagged_factorisation_pays_on_the_model():
    (y0, s0), (y1, s1, _tr) = help_models()
    print("gamma", HELP["gamma"], "steps without", s0["iterations"], "with the lagged ILU", s1["iterations"])
    assert s0["flags"] == 0 and s1["flags"] == 0
    assert s0["iterations"] >= 4 * s1["iterations"]
    assert (s0["iterations"], s1["iterations"]) == (HELP["steps_without"], HELP["steps_with"])          # what profiles/jfnk_precond.md records
    _f, _x0, x1, b, _rl, _cp, _rv, _nz = help_system()
    for y in (y0, y1):
        assert JM.true_residual(HELP["family"], HELP["prm"], x1, 1.0, -HELP["gamma"], b, y) <= 10 * HELP["rtol"]


def test_the_entry_points_are_declared_exported_and_check_their_arguments():
    L = fd.lib.load()
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    for n in ("factor_async", "apply_async", "factor_status"):
        for pre in ("fd_", "fd32_"):          # both element builds
            assert re.search(r"^int %scsc_solver_%s\(" % (pre, n), hdr, re.M), (pre, n)
            assert hasattr(L, pre + "csc_solver_" + n) and pre + "csc_solver_" + n in fd.lib.EXPORTS
    assert re.search(r"^int fd_jfnk_solver_set_csc_preconditioner\(", hdr, re.M)
    assert "fd_jfnk_solver_set_csc_preconditioner" in fd.lib.EXPORTS and not hasattr(L, "fd32_jfnk_solver_set_csc_preconditioner")
    ARG = 1
    err = lambda: L.fd_last_error().decode()          # noqa: E731
    # the argument checks precede any use of a context: no handle, no device, nothing dereferenced
    for T in (fd.lib.typed(L, np.float64), fd.lib.typed(L, np.float32)):
        assert T.fd_csc_solver_factor_async(None, 1.0, -1.0, None) == ARG and "solver is NULL" in err()
        assert T.fd_csc_solver_apply_async(None, None, None) == ARG and "NULL" in err()
        assert T.fd_csc_solver_factor_status(None, None) == ARG and "solver is NULL" in err()
    assert L.fd_jfnk_solver_set_csc_preconditioner(None, None) == ARG and "solver is NULL" in err()
    assert L.fd_jfnk_solver_set_csc_preconditioner(None, C.c_void_p(8)) == ARG and "solver is NULL" in err()
