"""The matrix-free consumer on the CPU: the numpy model (tests/jfnk_model.py) against csc_gmres_model.solve with the stored product plugged
in, its deliberately wrong variants, the convergence cases, the accuracy of the model's answers against the analytic Jacobians, and the
new entry points' argument errors at the ABI.

Accuracy.  The solve stops when the estimate is <= rtol ||b||.  The operator differs from alpha I + beta J_exact by the quotient's
truncation (O(eps_fd |f''|)) and its rounding noise (about eps / eps_fd relative), both near 1e-8 here, so the true residual
||b - (alpha I + beta J_exact) y|| / ||b|| stays of the order of rtol = 1e-6; the bound the GPU test asserts is 4 x the worst value this
file measures per family (MODEL_WORST below restates them; profiles/jfnk_accuracy.md has the table)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_gmres_model as G
import csc_solve_model as M
import jfnk_cases as JK
import jfnk_model as JM
import test_cscgmres_model_cpu as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the worst true residual of the model's y per family over JK.CONVERGENCE (test_model_accuracy_... recomputes and compares)
MODEL_WORST = {"tridiag": 5.70e-7, "tridiag_nl": 5.72e-7, "lap5": 3.07e-7, "lap5_nl": 3.81e-7}


@pytest.fixture(scope="module", autouse=True)
def _the_library_has_the_consumer():
    """These tests need only numpy, yet they describe fd_jfnk_*: a tree without those entry points has nothing the model is a model
    of, and a model that passed there would claim a consumer that does not exist.  So the module asks the built library for them first
    (one build, shared with the ABI test below) and every test here fails where they are missing."""
    fd.lib.build()
    assert hasattr(fd.lib.load(), "fd_jfnk_solve_async") and hasattr(fd, "JfnkSolver")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name,restart", [("lap5", 5), ("tridiag", 30), ("band", 2), ("odd", 64), ("lap5", 1)])
def test_the_cycle_is_csc_gmres_models_with_the_stored_product(name, restart):
    c = H.make_case(name)
    rl, nz, b, gamma = c["rl"], c["nz"], c["b"], c["gamma"]
    for maxit, keep in ((400, False), (7, True)):
        tr, tw = {}, {}
        want, wst = G.solve(rl, 1.0, -gamma, nz, b, 1e-10, maxit, keep_unconverged=keep, restart=restart, trace=tw)
        d = np.where(rl.diag >= 0, 1.0 - gamma * nz[np.maximum(rl.diag, 0)], 1.0)
        got, st = JM.gmres(lambda v, kind, j: M.matvec(rl, 1.0, -gamma, nz, v), lambda v: v / d, False, b, 1e-10, maxit, keep, restart, trace=tr)
        assert st == wst and np.array_equal(_bits(got), _bits(want))
        assert tr["len"] == tw["len"] and np.array_equal(_bits(tr["V"]), _bits(tw["V"])) and np.array_equal(_bits(tr["H"]), _bits(tw["H"]))


def test_every_fault_changes_a_compared_bit():
    cases = [JK.CONVERGENCE[1], JK.CONVERGENCE[3], JK.CASES[5]]
    for fault in JM.FAULTS[1:]:
        differs = False
        for c in cases:
            tr, tf = {}, {}
            y, st = JK.model(c, trace=tr)
            yf, sf = JK.model(c, fault=fault, trace=tf)
            differs = differs or st != sf or not np.array_equal(_bits(y), _bits(yf)) or not np.array_equal(_bits(tr["H"]), _bits(tf["H"]))
        assert differs, fault


@pytest.mark.parametrize("case", JK.CONVERGENCE, ids=lambda c: c["id"])
def test_convergence_cases_end_with_flags_0_and_are_accurate(case):
    tr = {}
    y, st = JK.model(case, trace=tr)
    f, x, b, d = JK.system(case["family"], case["prm"])
    res = JM.true_residual(case["family"], case["prm"], x, 1.0, -JK.GAMMA, b, y)
    print(case["id"], st, "cycles", len(tr["gammas"]), "true residual %.3e" % res)
    assert st["flags"] == 0 and 1 <= st["iterations"] < case["maxit"]
    assert res <= MODEL_WORST[case["family"]]
    if case["id"].startswith("tridiag_nl-1025"):
        assert len(tr["gammas"]) >= 3


def test_first_column_meets_a_loose_rtol_and_b_zero():
    c = JK.CONVERGENCE[0]
    y, st = JK.model(c, rtol=0.9)
    assert st["flags"] == 0 and st["iterations"] == 1
    y, st = JK.model(c, b=np.zeros(255))
    assert st == {"flags": 0, "iterations": 0, "resid": 0.0, "bnorm": 0.0} and np.array_equal(y, np.zeros(255))


def test_failures_of_the_model():
    c = JK.CONVERGENCE[3]          # lap5 9x7 with the diagonal
    f, x, b, d = JK.system(c["family"], c["prm"])
    for bad in (0.0, np.inf):
        dd = d.copy(); dd[11] = bad
        y, st = JK.model(c, d=dd, keep=False)
        assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    bb = b.copy(); bb[3] = np.nan
    y, st = JK.model(c, b=bb, keep=False)
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    xx = x.copy(); xx[5] = np.nan
    y, st = JK.model(c, x=xx, keep=False)
    assert st["flags"] == 2 and np.all(np.isnan(y))
    y, st = JK.model(c, x=xx, keep=True)
    assert st["flags"] == 2 and np.array_equal(y, np.zeros(x.size))


def test_the_entry_points_are_declared_exported_and_check_their_arguments():
    fd.lib.build()
    L = fd.lib.load()
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    names = ("solver_create", "solver_destroy", "solver_set_options", "solver_set_policy", "solver_set_steps", "solver_set_lazy_f",
             "solver_set_diagonal", "apply_async", "solve_async", "solver_status", "solver_counts", "solver_basis")
    for n in names:
        assert re.search(r"^int fd_jfnk_%s\(" % n, hdr, re.M), n
        assert hasattr(L, "fd_jfnk_" + n) and "fd_jfnk_" + n in fd.lib.EXPORTS
        assert not hasattr(L, "fd32_jfnk_" + n) and "fd32_jfnk_" + n not in fd.lib.EXPORTS          # Float64 only
    ARG = 1
    err = lambda: L.fd_last_error().decode()          # noqa: E731
    h = C.c_void_p()
    assert L.fd_jfnk_solver_create(None, 10, 0, 30, C.byref(h)) == ARG and "NULL" in err()
    assert L.fd_jfnk_solver_destroy(None) == 0
    assert L.fd_jfnk_solver_set_options(None, 1e-6, 10) == ARG and "solver is NULL" in err()
    assert L.fd_jfnk_solver_set_policy(None, 1) == ARG
    assert L.fd_jfnk_solver_set_steps(None, -1.0, -1.0, 1.0) == ARG
    assert L.fd_jfnk_solver_set_lazy_f(None, fd.lib.F_LAUNCH_LAZY_JVP(), 0) == ARG
    assert L.fd_jfnk_solver_set_diagonal(None, None) == ARG
    assert L.fd_jfnk_apply_async(None, 1.0, -1.0, fd.lib.F_LAUNCH(), None, None, None, None, None) == ARG and "NULL" in err()
    assert L.fd_jfnk_solve_async(None, 1.0, -1.0, fd.lib.F_LAUNCH(), None, None, None, None, None) == ARG and "NULL" in err()
    assert L.fd_jfnk_solver_status(None, None, None, None, None) == ARG
    assert L.fd_jfnk_solver_counts(None, None, None) == ARG
    assert L.fd_jfnk_solver_basis(None, None, None, None, None) == ARG
    # the range checks come before the device is touched (fd_jfnk_solver_create keeps them ahead of its first use of ctx, and says so):
    # a context that is never dereferenced stands in for one
    fake = C.c_void_p(8)
    assert L.fd_jfnk_solver_create(fake, 0, 0, 30, C.byref(h)) == 2 and "N = 0" in err()                     # FD_ERR_SHAPE
    assert L.fd_jfnk_solver_create(fake, 2 ** 31, 0, 30, C.byref(h)) == 2
    assert L.fd_jfnk_solver_create(fake, 10, 2, 30, C.byref(h)) != 0 and "complex-mode" in err()             # the JVP's message
    assert L.fd_jfnk_solver_create(fake, 10, 0, 0, C.byref(h)) == ARG and "restart = 0" in err()
    assert L.fd_jfnk_solver_create(fake, 10, 1, 65, C.byref(h)) == ARG and "restart = 65" in err()
    assert h.value is None
