"""The warm start on the CPU: tests/warm_model.py pinned to the existing models bit for bit (y0 = None and y0 = zeros give what
csc_solve_model / csc_block_model / csc_ilu_model / csc_gmres_model / jfnk_model / jfnk_pc_model give: b - (alpha 0 + beta 0) = b for a
finite J, so the restated recurrences ARE the yardsticks' wherever they can be compared), deliberately wrong variants of the model (which
the inputs of tests/test_gpu_warm_start.py must expose), the condition that the implicit-step sequence of the GPU test saves
iterations in the model, and the new symbols at the ABI."""
import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_block_model as BM
import csc_gmres_model as G
import csc_ilu_model as IM
import csc_solve_model as M
import jfnk_cases as JK
import jfnk_model as JM
import jfnk_pc_cases as PC
import jfnk_pc_model as PM
import warm_cases as WC
import warm_model as W


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _same_status(a, b):
    return all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in ("flags", "iterations", "resid", "bnorm")) and set(a) == set(b)


# ---- 1. pinned to the existing models ----------------------------------------------------------------------------------------------------
def _pin_systems():
    out = {}
    for name, (colptr, rowval, N) in (("lap5", M.lap5_pattern(9, 7)), ("band", M.random_band_pattern(400, 20, 5, 3)),
                                      ("odd", M.odd_pattern(500, 77, 60, 1))):
        rng = np.random.default_rng(5)
        nz, b = rng.uniform(-1.0, 1.0, rowval.size), rng.uniform(-1.0, 1.0, N)
        rows = np.zeros(N)
        np.add.at(rows, rowval, np.abs(nz))
        out[name] = (M.RowLists(colptr, rowval, N), nz, b, 1.0, -float(0.9 / rows.max()))
    colptr, rowval, nz, N = BM.reaction_diffusion(3, 3, 5, 10.0, 10.0, 0.3, 2)
    out["react"] = (M.RowLists(colptr, rowval, N), nz, np.random.default_rng(102).standard_normal(N), 1.0, -0.1)
    return out


PIN = _pin_systems()
PIN_PRECONDS = (("jacobi",), ("block", 5), ("ilu", 7))


def _existing(rl, alpha, beta, nz, b, method, precond, rtol, maxit, keep):
    if method == "gmres":
        return G.solve(rl, alpha, beta, nz, b, rtol, maxit, keep, restart=5, precond=precond)
    if precond[0] == "ilu":
        return IM.solve(rl, alpha, beta, nz, b, rtol, maxit, keep, bs=precond[1])
    return BM.solve(rl, alpha, beta, nz, b, rtol, maxit, keep, precond=precond)          # (("jacobi",): csc_solve_model.solve)


@pytest.mark.parametrize("name", sorted(PIN))
@pytest.mark.parametrize("method", WC.METHODS)
@pytest.mark.parametrize("precond", PIN_PRECONDS, ids=lambda p: "".join(map(str, p)))
def test_the_sparse_recurrences_are_the_existing_models_bit_for_bit(name, method, precond):
    rl, nz, b, alpha, beta = PIN[name]
    assert rl.nlong == (1 if name == "odd" else 0)
    for dtype, rtol, maxit, keep in ((np.float64, 1e-10, 60, False), (np.float32, 1e-6, 60, False), (np.float64, 0.0, 7, True), (np.float64, 0.0, 7, False)):
        nzt, bt = nz.astype(dtype), b.astype(dtype)
        want, wst = _existing(rl, alpha, beta, nzt, bt, method, precond, rtol, maxit, keep)
        assert wst["iterations"] >= 1
        for y0 in (None, np.zeros(rl.N, dtype=dtype)):
            got, st = W.csc_solve(rl, alpha, beta, nzt, bt, y0, method, precond, 5, rtol, maxit, keep)
            assert st == wst and _same(got, want), (dtype, rtol, y0 is None)
    # the ends before the first step: b = 0, a NaN in b, a zero pivot
    bad_nz = nz.copy()
    bad_nz[rl.diag[np.nonzero(rl.diag >= 0)[0][0]]] = 1.0 / -beta          # 1 + beta / -beta = 0 on the diagonal
    nan_b = b.copy()
    nan_b[3] = np.nan
    for nzv, bv in ((nz, np.zeros(rl.N)), (nz, nan_b), (bad_nz, b)):
        for keep in (False, True):
            want, wst = _existing(rl, alpha, beta, nzv, bv, method, precond, 1e-10, 9, keep)
            for y0 in (None, np.zeros(rl.N)):
                got, st = W.csc_solve(rl, alpha, beta, nzv, bv, y0, method, precond, 5, 1e-10, 9, keep)
                assert _same_status(st, wst) and _same(got, want)


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("family,prm", [("tridiag_nl", (65,)), ("lap5_nl", (7, 9)), ("tridiag", (2,))])
def test_the_matrix_free_recurrence_is_the_existing_models_bit_for_bit(family, prm, fdtype):
    f, x, b, d = JK.system(family, prm)
    zeros = np.zeros(x.size)
    for dd in (None, d):
        for rtol, maxit, keep in ((JK.RTOL, 40, False), (0.0, 7, True)):
            tr = {}
            want, wst = JM.solve(f, x, b, 1.0, -JK.GAMMA, fdtype, dd, rtol, maxit, keep, 5, trace=tr)
            for y0 in (None, zeros):
                tw = {}
                got, st = W.jfnk_solve(f, x, b, 1.0, -JK.GAMMA, y0, fdtype, dd, None, rtol, maxit, keep, 5, trace=tw)
                assert st == wst and _same(got, want)
                assert tw["applications"] == tr["applications"] + (0 if y0 is None else 1)
    colptr, rowval, rl, _x0, nz0 = PC.stored(family, prm)
    for kind in (("jacobi",), ("block", 5), ("ilu", 64)):
        want, wst = PM.solve(f, x, b, 1.0, -PC.GAMMA, rl, (1.0, -PC.GAMMA0, nz0), kind, fdtype, JK.RTOL, 40, False, 5)
        for y0 in (None, zeros):
            got, st = W.jfnk_solve(f, x, b, 1.0, -PC.GAMMA, y0, fdtype, None, (rl, (1.0, -PC.GAMMA0, nz0), kind), JK.RTOL, 40, False, 5)
            assert st == wst and _same(got, want)


# ---- 2. the GPU test's inputs expose a wrong start -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", [f for f in W.FAULTS if f])
def test_every_fault_is_told_apart_by_an_input_of_the_gpu_test(fault):
    seen = 0
    for name, method, precond, dtype in WC.SPARSE_CASES:
        if fault == "rhat_b" and method != "bicgstab":
            continue
        _c, _r, _N, nz, b, y0, gamma, rl = WC.system(name)
        nzt, bt, y0t = nz.astype(dtype), b.astype(dtype), y0.astype(dtype)
        args = (rl, 1.0, -gamma, nzt, bt, y0t, method, precond, WC.RESTART, WC.rtol_of(dtype), WC.MAXIT, True)
        right, rst = W.csc_solve(*args)
        wrong, wst = W.csc_solve(*args, fault=fault)
        seen += int(not _same(right, wrong) or rst != wst)
    assert seen >= 1
    for method in WC.METHODS:                    # and the sequence's first warm step, on either method
        if fault == "rhat_b" and method != "bicgstab":
            continue
        _c, _r, _N, nz, u0, rl = WC.sequence()
        right, rst = W.csc_solve(rl, 1.0, -WC.SEQ_GAMMA, nz, u0, u0, method, rtol=WC.SEQ_RTOL)
        wrong, wst = W.csc_solve(rl, 1.0, -WC.SEQ_GAMMA, nz, u0, u0, method, rtol=WC.SEQ_RTOL, fault=fault)
        assert not _same(right, wrong) or rst != wst
    told = 0
    for case in WC.JFNK_CASES:                   # the matrix-free consumer has no shadow residual
        if fault == "rhat_b":
            continue
        f, x, b, d, y0 = WC.jfnk_system(case["family"], case["prm"])
        kw = dict(fdtype=case["fdtype"], d=d if case["pc"] == "diag" else None, lent=WC.jfnk_lent(case) if case["kind"] else None, rtol=case["rtol"],
                  max_iterations=case["maxit"], keep_unconverged=True, restart=case["restart"])
        right, rst = W.jfnk_solve(f, x, b, 1.0, -JK.GAMMA, y0, **kw)
        wrong, wst = W.jfnk_solve(f, x, b, 1.0, -JK.GAMMA, y0, fault=fault, **kw)
        told += int(not _same(right, wrong) or rst != wst)
    assert told >= 1 or fault == "rhat_b"


# ---- 3. the sequence saves iterations: a condition of the GPU test, checked here ------------------------------------------------------------
def sequence_counts(method="bicgstab"):
    """[(cold iterations, warm iterations)] per step of warm_cases.sequence() in the model; the state follows the cold solves."""
    _c, _r, _N, nz, u, rl = WC.sequence()
    out = []
    for _step in range(WC.SEQ_STEPS):
        cold, cst = W.csc_solve(rl, 1.0, -WC.SEQ_GAMMA, nz, u, None, method, rtol=WC.SEQ_RTOL)
        _warm, wst = W.csc_solve(rl, 1.0, -WC.SEQ_GAMMA, nz, u, u, method, rtol=WC.SEQ_RTOL)
        assert cst["flags"] == 0 and wst["flags"] == 0
        out.append((cst["iterations"], wst["iterations"]))
        u = cold
    return out


def test_the_implicit_step_sequence_saves_iterations_in_the_model():
    counts = sequence_counts()
    print(counts)
    assert len(counts) == 4 and WC.SEQ_GRID == (12, 11)
    assert all(cold >= 10 for cold, _w in counts)
    assert all(warm < cold for cold, warm in counts[1:])


# ---- 4. the ends of a warm start in the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", WC.METHODS)
def test_the_rules_of_the_start(method):
    _c, _r, N, nz, b, y0, gamma, rl = WC.system("lap5")
    args = dict(method=method, restart=WC.RESTART, max_iterations=200)
    tight, tst = W.csc_solve(rl, 1.0, -gamma, nz, b, y0, rtol=1e-12, **args)
    assert tst["flags"] == 0
    again, ast = W.csc_solve(rl, 1.0, -gamma, nz, b, tight, rtol=1e-8, **args)          # good enough by construction: y = y0 exactly
    assert ast["flags"] == 0 and ast["iterations"] == 0 and _same(again, tight) and 0.0 < ast["resid"] <= 1e-8 * ast["bnorm"]
    _y, st = W.csc_solve(rl, 1.0, -gamma, nz, b, tight, rtol=1e-12, **args)              # the converged y as y0: at most one more
    assert st["flags"] == 0 and st["iterations"] <= 1
    y, st = W.csc_solve(rl, 1.0, -gamma, nz, np.zeros(N), y0, rtol=1e-10, **args)        # b = 0: y = 0 whatever y0 holds
    assert st == {"flags": 0, "iterations": 0, "resid": 0.0, "bnorm": 0.0} and not y.any()
    bad = y0.copy()
    bad[5] = np.nan
    y, st = W.csc_solve(rl, 1.0, -gamma, nz, b, bad, rtol=1e-10, **args)
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    y, st = W.csc_solve(rl, 1.0, -gamma, nz, b, bad, rtol=1e-10, keep_unconverged=True, **args)
    assert st["flags"] == 2 and _same(y, bad)


# ---- 5. the ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_and_check_their_arguments():
    L = fd.lib.load()
    for name in ("fd_csc_solve_from_async", "fd32_csc_solve_from_async", "fd_jfnk_solve_from_async"):
        assert hasattr(L, name), name
    assert L.fd_csc_solve_from_async(None, 1.0, -1.0, None, None, None, None) == 1 and b"NULL" in L.fd_last_error()
    assert L.fd_jfnk_solve_from_async(None, 1.0, -1.0, fd.lib.F_LAUNCH(), None, None, None, None, None, None) == 1 and b"NULL" in L.fd_last_error()
    import inspect
    assert "y0" in inspect.signature(fd.CscSolver.solve).parameters and "y0" in inspect.signature(fd.JfnkSolver.solve).parameters
