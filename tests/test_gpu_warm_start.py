"""The warm start of the sparse and the matrix-free consumer on the device (fd_csc_solve_from_async, fd_jfnk_solve_from_async;
solve(..., y0=) in Python): y, flags, iterations, resid and ||b|| BIT FOR BIT against tests/warm_model.py over the inputs of
tests/warm_cases.py; the y0 variants that must equal the cold start; the ends of a warm start; aliasing with guard bands around every
array; a capped solve continued in place; the iteration counts of the implicit-step sequence; the matrix-free consumer's counts.

Every case is a few device solves of at most 2049 unknowns; the model's answer is computed once per case."""
import os
import re
import subprocess

import numpy as np
import pytest

import finitediff_jl_amd as fd
import jfnk_cases as JK
import jfnk_model as JM
import jfnk_pc_cases as PC
import test_cscblock_model_cpu as HB
import test_jfnk_model_cpu as HJ
import test_warm_model_cpu as HW
import warm_cases as WC
import warm_model as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, BAND = 7.25, 8          # a guard band of 8 elements on either side keeps every array on a 16-byte boundary


def _guarded(a, dtype=np.float64, off=0):
    """a on the device between guard bands; off = 1 puts it one element further on: off a 16-byte pair."""
    a = np.ascontiguousarray(a, dtype=dtype)
    buf = torch.full((a.size + 2 * BAND + off,), CANARY, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    buf[BAND + off:BAND + off + a.size] = torch.as_tensor(a, device="cuda")
    return buf, buf[BAND + off:BAND + off + a.size]


def _intact(buf, a=None, off=0):
    """The guard bands of buf are untouched and (a given) its body still holds a bit for bit."""
    h = buf.cpu().numpy()
    ok = bool(np.all(h[:BAND + off] == CANARY) and np.all(h[-BAND:] == CANARY))
    return ok and (a is None or HW._same(h[BAND + off:-BAND], np.ascontiguousarray(a, dtype=h.dtype)))


def _select(s, precond):
    if precond[0] == "jacobi":
        s.set_preconditioner("jacobi")
    elif precond[0] == "block":
        s.set_preconditioner("block_jacobi", precond[1])
    else:
        s.set_block_ilu(precond[1])


def _sparse_solver(name, method, precond, dtype, rtol=None, maxit=WC.MAXIT, keep=True):
    colptr, rowval, N = WC.system(name)[:3]
    s = fd.CscSolver((colptr.astype(np.int64), rowval.astype(np.int64), N), dtype=dtype, idx_base=0)
    _select(s, precond)
    s.set_method(method, WC.RESTART)
    s.set_options(WC.rtol_of(dtype) if rtol is None else rtol, maxit)
    s.set_policy(keep)
    return s


def _status_same(a, b):
    return HW._same_status(a, b)


# ---- 1. the sparse consumer: bit identity, the cold variants, aliasing ---------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.SPARSE_CASES, ids=lambda c: "%s-%s-%s-%s" % (c[0], c[1], "".join(map(str, c[2])), np.dtype(c[3]).name))
def test_sparse_warm_solve_equals_the_model_bit_for_bit(case):
    name, method, precond, dtype = case
    _c, _r, N, nz, b, y0, gamma, rl = WC.system(name)
    nzt, bt, y0t = nz.astype(dtype), b.astype(dtype), y0.astype(dtype)
    want, wst = W.csc_solve(rl, 1.0, -gamma, nzt, bt, y0t, method, precond, WC.RESTART, WC.rtol_of(dtype), WC.MAXIT, True)
    s = _sparse_solver(name, method, precond, dtype)
    nzb, nzd = _guarded(nzt, dtype)
    bb, bd = _guarded(bt, dtype)
    y0b, y0d = _guarded(y0t, dtype)
    yb, yd = _guarded(np.full(N, CANARY), dtype)
    s.solve(nzd, bd, yd, 1.0, -gamma, y0=y0d)
    st = s.status()
    got = yd.cpu().numpy()
    print(case[0], method, precond, np.dtype(dtype).name, st, wst)
    assert st == wst and HW._same(got, want)
    assert _intact(nzb, nzt) and _intact(bb, bt) and _intact(y0b, y0t) and _intact(yb)
    # y0 is y: continued in place; the bits of the call above
    yb2, yd2 = _guarded(y0t, dtype)
    s.solve(nzd, bd, yd2, 1.0, -gamma, y0=yd2)
    assert s.status() == st and HW._same(yd2.cpu().numpy(), got) and _intact(yb2) and _intact(bb, bt)
    # y0 is b, and y is b: the bits of the call with copies
    wantb, wstb = W.csc_solve(rl, 1.0, -gamma, nzt, bt, bt, method, precond, WC.RESTART, WC.rtol_of(dtype), WC.MAXIT, True)
    s.solve(nzd, bd, yd, 1.0, -gamma, y0=bd)
    assert s.status() == wstb and HW._same(yd.cpu().numpy(), wantb) and _intact(bb, bt) and _intact(yb)
    bb2, bd2 = _guarded(bt, dtype)
    s.solve(nzd, bd2, bd2, 1.0, -gamma, y0=y0d)
    assert s.status() == st and HW._same(bd2.cpu().numpy(), got) and _intact(bb2) and _intact(y0b, y0t) and _intact(nzb, nzt)
    # the cold start three ways: the existing entry point, y0 = NULL through the new one, y0 all +0.0
    s.solve(nzd, bd, yd, 1.0, -gamma)
    cst, cold = s.status(), yd.cpu().numpy()
    wantc, wstc = W.csc_solve(rl, 1.0, -gamma, nzt, bt, None, method, precond, WC.RESTART, WC.rtol_of(dtype), WC.MAXIT, True)
    assert cst == wstc and HW._same(cold, wantc)
    yd.fill_(CANARY)
    fd.lib.check(s.Lt.fd_csc_solve_from_async(s.handle, 1.0, -gamma, nzd.data_ptr(), bd.data_ptr(), None, yd.data_ptr()))
    assert s.status() == cst and HW._same(yd.cpu().numpy(), cold)
    zb, zd = _guarded(np.zeros(N), dtype)
    yd.fill_(CANARY)
    s.solve(nzd, bd, yd, 1.0, -gamma, y0=zd)
    assert s.status() == cst and HW._same(yd.cpu().numpy(), cold) and _intact(zb, np.zeros(N)) and _intact(yb)


# ---- 2. the ends of a warm start ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", WC.METHODS)
@pytest.mark.parametrize("precond", WC.PRECONDS, ids=lambda p: "".join(map(str, p)))
def test_sparse_edges_of_the_start(method, precond):
    name, dtype = "lap5", np.float64
    _c, _r, N, nz, b, y0, gamma, rl = WC.system(name)
    nzd, bd, y0d = _guarded(nz)[1], _guarded(b)[1], _guarded(y0)[1]
    yb, yd = _guarded(np.full(N, CANARY))

    def both(rtol, bv, bdev, y0v, y0dev, keep=False, nzv=nz, nzdev=nzd, maxit=200):
        want, wst = W.csc_solve(rl, 1.0, -gamma, nzv, bv, y0v, method, precond, WC.RESTART, rtol, maxit, keep)
        s = _sparse_solver(name, method, precond, dtype, rtol, maxit, keep)
        yd.fill_(CANARY)
        s.solve(nzdev, bdev, yd, 1.0, -gamma, y0=y0dev)
        st, got = s.status(), yd.cpu().numpy()
        assert _status_same(st, wst) and HW._same(got, want) and _intact(yb), (st, wst)
        return got, st

    tight, tst = both(1e-12, b, bd, y0, y0d)
    assert tst["flags"] == 0
    tightd = _guarded(tight)[1]
    again, ast = both(1e-8, b, bd, tight, tightd)                      # ||r0|| <= rtol ||b|| by construction
    assert ast["flags"] == 0 and ast["iterations"] == 0 and HW._same(again, tight)
    _y, st = both(1e-12, b, bd, tight, tightd)                        # the converged y of a previous solve
    assert st["flags"] == 0 and st["iterations"] <= 1
    zero = np.zeros(N)
    y, st = both(1e-10, zero, _guarded(zero)[1], y0, y0d)             # b = 0 with y0 != 0
    assert st == {"flags": 0, "iterations": 0, "resid": 0.0, "bnorm": 0.0} and not y.any()
    bad = y0.copy()
    bad[5] = np.nan
    badd = _guarded(bad)[1]
    y, st = both(1e-10, b, bd, bad, badd)
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    y, st = both(1e-10, b, bd, bad, badd, keep=True)
    assert st["flags"] == 2 and HW._same(y, bad)
    nzbad = nz.copy()                                                 # row 0 of A is zero inside every leading block: a zero pivot
    cols = np.repeat(np.arange(N), np.diff(rl.colptr))
    nzbad[rl.diag[0]] = 1.0 / gamma
    nzbad[np.nonzero((rl.rowval == 0) & (cols == 1))[0][0]] = 0.0
    assert 1.0 - gamma * nzbad[rl.diag[0]] == 0.0
    y, st = both(1e-10, b, bd, y0, y0d, nzv=nzbad, nzdev=_guarded(nzbad)[1])
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))


# ---- 3. continuation and the sequence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", WC.METHODS)
def test_a_capped_sparse_solve_is_continued_in_place_to_convergence(method):
    """max_iterations = 3 under the keep policy, then y0 is y until flags = 0; the true residual in extended precision meets the bound
    of the cold block-Jacobi solve on a stored reaction-diffusion Jacobian (tests/test_gpu_cscblock.py: 10 RTOL)."""
    colptr, rowval, nz, N, b = HB.family_case(4, 12, 10, 1e3, 1e3, 0.3)
    s = fd.CscSolver((colptr.astype(np.int64), rowval.astype(np.int64), N), idx_base=0)
    s.set_preconditioner("block_jacobi", 4)
    s.set_method(method, WC.RESTART)
    s.set_options(HB.RTOL, 3)
    s.set_policy(True)
    nzd, bd = _guarded(nz)[1], _guarded(b)[1]
    yb, yd = _guarded(np.full(N, CANARY))
    s.solve(nzd, bd, yd, 1.0, -HB.GAMMA)
    st, calls, total = s.status(), 1, 3
    assert st["flags"] == 1 and st["iterations"] == 3
    while st["flags"] == 1 and calls < 400:
        s.solve(nzd, bd, yd, 1.0, -HB.GAMMA, y0=yd)
        st = s.status()
        calls, total = calls + 1, total + st["iterations"]
    res = HB.true_residual(colptr, rowval, nz, N, 1.0, -HB.GAMMA, yd.cpu().numpy(), b)
    print("%s: %d calls, %d iterations, true residual %.3e, bound %.3e" % (method, calls, total, res, 10 * HB.RTOL))
    assert st["flags"] == 0 and calls >= 2 and _intact(yb)
    assert res <= 10 * HB.RTOL


def test_the_sequence_needs_the_models_iterations_cold_and_warm():
    counts = HW.sequence_counts()
    assert all(w < c for c, w in counts[1:])                          # (tests/test_warm_model_cpu.py: the condition)
    colptr, rowval, N, nz, u, rl = WC.sequence()
    s = fd.CscSolver((colptr, rowval, N), idx_base=0)
    s.set_options(WC.SEQ_RTOL, 500)
    nzd = _guarded(nz)[1]
    ud = _guarded(u)[1]
    cold, warm = _guarded(np.zeros(N))[1], _guarded(np.zeros(N))[1]
    got = []
    for _step in range(WC.SEQ_STEPS):
        s.solve(nzd, ud, cold, 1.0, -WC.SEQ_GAMMA)
        c = s.status()
        s.solve(nzd, ud, warm, 1.0, -WC.SEQ_GAMMA, y0=ud)
        w = s.status()
        assert c["flags"] == 0 and w["flags"] == 0
        got.append((c["iterations"], w["iterations"]))
        ud.copy_(cold)
    print(got, counts)
    assert got == counts


# ---- 4. the matrix-free consumer -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lend(case):
    colptr, rowval, rl, _x0, nz0 = PC.stored(case["family"], case["prm"])
    pc = fd.CscSolver((colptr, rowval, rl.N), idx_base=0)
    _select(pc, case["kind"])
    pc.factor(torch.as_tensor(np.ascontiguousarray(nz0), device="cuda"), 1.0, -PC.GAMMA0)
    return pc


def _jf_solver(case, d=None, rtol=None, maxit=None, keep=True):
    s = fd.JfnkSolver(JK.size_of(case["family"], case["prm"]), case["fdtype"], case["restart"])
    s.set_options(case["rtol"] if rtol is None else rtol, case["maxit"] if maxit is None else maxit)
    s.set_policy(keep)
    if case["pc"] == "diag":
        s.set_diagonal(d)
    elif case["kind"]:
        s.set_preconditioner(_lend(case))
    return s


def _jf_model(case, num_cus, y0, b=None, d=None, rtol=None, maxit=None, keep=True, trace=None):
    f, x, b0, d0, _y0 = WC.jfnk_system(case["family"], case["prm"])
    return W.jfnk_solve(f, x, b0 if b is None else b, 1.0, -JK.GAMMA, y0, case["fdtype"], (d0 if d is None else d) if case["pc"] == "diag" else None,
                        WC.jfnk_lent(case) if case["kind"] else None, case["rtol"] if rtol is None else rtol,
                        case["maxit"] if maxit is None else maxit, keep, case["restart"], num_cus, trace=trace)


@pytest.mark.parametrize("case", WC.JFNK_CASES, ids=lambda c: c["id"])
def test_matrix_free_warm_solve_equals_the_model_bit_for_bit(num_cus, case):
    _f, x, b, d, y0 = WC.jfnk_system(case["family"], case["prm"])
    N = x.size
    f = fd.BuiltinF(case["family"], *case["prm"])
    xb, xd = _guarded(x)
    bb, bd = _guarded(b)
    db, dd = _guarded(d)
    y0b, y0d = _guarded(y0)
    yb, yd = _guarded(np.full(N, CANARY))
    s = _jf_solver(case, dd)
    want, wst = _jf_model(case, num_cus, y0)
    s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA, y0=y0d)
    st, got = s.status(), yd.cpu().numpy()
    print(case["id"], st, wst)
    assert st == wst and HW._same(got, want)
    assert _intact(xb, x) and _intact(bb, b) and _intact(db, d) and _intact(y0b, y0) and _intact(yb)
    yb2, yd2 = _guarded(y0)                                            # y0 is y
    s.solve(f, xd, bd, yd2, 1.0, -JK.GAMMA, y0=yd2)
    assert s.status() == st and HW._same(yd2.cpu().numpy(), got) and _intact(yb2)
    for src, srcd in ((b, bd), (x, xd)):                              # y0 is b; y0 is x
        wanta, wsta = _jf_model(case, num_cus, src)
        s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA, y0=srcd)
        assert s.status() == wsta and HW._same(yd.cpu().numpy(), wanta)
    bb2, bd2 = _guarded(b)                                            # y is b
    s.solve(f, xd, bd2, bd2, 1.0, -JK.GAMMA, y0=y0d)
    assert s.status() == st and HW._same(bd2.cpu().numpy(), got) and _intact(bb2)
    assert _intact(xb, x) and _intact(bb, b) and _intact(y0b, y0)
    # the cold start three ways
    s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA)
    cst, cold = s.status(), yd.cpu().numpy()
    wantc, wstc = _jf_model(case, num_cus, None)
    assert cst == wstc and HW._same(cold, wantc)
    fn, fctx = s._launcher(f)
    yd.fill_(CANARY)
    fd.lib.check(s.ctx.L.fd_jfnk_solve_from_async(s.handle, 1.0, -JK.GAMMA, fn, fctx, xd.data_ptr(), None, bd.data_ptr(), None, yd.data_ptr()))
    assert s.status() == cst and HW._same(yd.cpu().numpy(), cold)
    yd.fill_(CANARY)
    s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA, y0=_guarded(np.zeros(N))[1])
    assert s.status() == cst and HW._same(yd.cpu().numpy(), cold)


@pytest.mark.parametrize("fdtype", ["forward", "central"])
def test_matrix_free_counts_and_edges(num_cus, fdtype):
    case = WC._jf("tridiag_nl", (1025,), fdtype, "diag")
    _f, x, b, d, y0 = WC.jfnk_system(case["family"], case["prm"])
    N = x.size
    f = fd.BuiltinF(case["family"], *case["prm"])
    xd, bd, dd, y0d = _guarded(x)[1], _guarded(b)[1], _guarded(d)[1], _guarded(y0)[1]
    yb, yd = _guarded(np.full(N, CANARY))
    base = 1 if fdtype == "forward" else 0
    # rtol = 0: nothing converges, the host enqueues 12 steps and a residual per cycle end (5, 5, 2); the warm start adds ONE application
    s = _jf_solver(case, dd, rtol=0.0, maxit=12)
    c0 = s.counts()
    s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA)
    c1 = s.counts()
    s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA, y0=y0d)
    c2 = s.counts()
    tr = {}
    want, wst = _jf_model(case, num_cus, y0, rtol=0.0, maxit=12, trace=tr)
    assert s.status() == wst and HW._same(yd.cpu().numpy(), want)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (15, base) and (c2[0] - c1[0], c2[1] - c1[1]) == (16, base)
    trc = {}
    _jf_model(case, num_cus, None, rtol=0.0, maxit=12, trace=trc)          # (the model stops where the device idles: no residual behind the last cycle)
    assert tr["applications"] == trc["applications"] + 1 == 15 and tr["base_evaluations"] == trc["base_evaluations"] == base

    def both(bv, y0v, dv=d, keep=False, rtol=JK.RTOL):
        s = _jf_solver(case, _guarded(dv)[1], rtol=rtol, maxit=60, keep=keep)
        tr = {}
        want, wst = _jf_model(case, num_cus, y0v, b=bv, d=dv, rtol=rtol, maxit=60, keep=keep, trace=tr)
        before = s.counts()
        yd.fill_(CANARY)
        s.solve(f, xd, _guarded(bv)[1], yd, 1.0, -JK.GAMMA, y0=_guarded(y0v)[1])
        st, got, after = s.status(), yd.cpu().numpy(), s.counts()
        assert _status_same(st, wst) and HW._same(got, want) and _intact(yb), (st, wst)
        return got, st, (after[0] - before[0], after[1] - before[1]), tr

    tight, tst, _n, _t = both(b, y0, rtol=1e-9)
    assert tst["flags"] == 0
    again, ast, n, _t = both(b, tight, rtol=1e-5)                     # good enough by construction: one application, no step
    assert ast["flags"] == 0 and ast["iterations"] == 0 and HW._same(again, tight) and n[0] >= 1
    y, st, _n, _t = both(np.zeros(N), y0)                             # b = 0
    assert st["flags"] == 0 and st["iterations"] == 0 and not y.any()
    bad = y0.copy()
    bad[7] = np.nan
    y, st, _n, _t = both(b, bad)
    assert st["flags"] == 2 and np.all(np.isnan(y))
    y, st, _n, _t = both(b, bad, keep=True)
    assert st["flags"] == 2 and HW._same(y, bad)
    d0 = d.copy()                                                     # a bad pivot: nothing of the operator is enqueued or counted
    d0[3] = 0.0
    y, st, n, tr = both(b, y0, dv=d0)
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y)) and n == (0, 0)
    assert tr["applications"] == 0 and tr["base_evaluations"] == 0


def test_a_capped_matrix_free_solve_is_continued_in_place_to_convergence():
    """As the sparse consumer's, on a convergence case of tests/jfnk_cases.py with its bound (tests/test_gpu_jfnk.py: 4 x the model's worst)."""
    case = JK.CONVERGENCE[3]
    assert case["family"] == "lap5" and case["diag"] and not case["xoff"] and case["route"] == "plain"
    f0, x, b, d = JK.system(case["family"], case["prm"])
    N = x.size
    f = fd.BuiltinF(case["family"], *case["prm"])
    s = fd.JfnkSolver(N, case["fdtype"], case["restart"])
    s.set_options(case["rtol"], 3)
    s.set_policy(True)
    xd, bd, dd = _guarded(x)[1], _guarded(b)[1], _guarded(d)[1]
    s.set_diagonal(dd)
    yb, yd = _guarded(np.full(N, CANARY))
    s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA)
    st, calls = s.status(), 1
    assert st["flags"] == 1 and st["iterations"] == 3
    while st["flags"] == 1 and calls < 100:
        s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA, y0=yd)
        st, calls = s.status(), calls + 1
    res = JM.true_residual(case["family"], case["prm"], x, 1.0, -JK.GAMMA, b, yd.cpu().numpy())
    print("%d calls, true residual %.3e, bound %.3e" % (calls, res, 4 * HJ.MODEL_WORST[case["family"]]))
    assert st["flags"] == 0 and calls > 1 and _intact(yb)
    assert res <= 4 * HJ.MODEL_WORST[case["family"]]


@pytest.mark.parametrize("fdtype,pc,xoff", [("forward", None, 0), ("central", "diag", 0), ("forward", ("block", 5), 1)])
def test_matrix_free_y0_off_a_pair_takes_the_scalar_order(monkeypatch, num_cus, fdtype, pc, xoff):
    """The start's application reads y0 where the caller put it: one double off a 16-byte boundary the dot of (x, y0) runs in the
    scalar order (FDJAC_SMALL=0: the large kernels at N = 1025) and the closing kernel in its unpaired variant."""
    monkeypatch.setenv("FDJAC_SMALL", "0")
    case = WC._jf("tridiag_nl", (1025,), fdtype, pc)
    f0, x, b, d, y0 = WC.jfnk_system(case["family"], case["prm"])
    f = fd.BuiltinF(case["family"], *case["prm"])
    xb, xd = _guarded(x, off=xoff)
    bd, dd = _guarded(b)[1], _guarded(d)[1]
    y0b, y0d = _guarded(y0, off=1)
    yb, yd = _guarded(np.full(x.size, CANARY))
    assert y0d.data_ptr() % 16 == 8 and (xd.data_ptr() % 16 == 0) == (not xoff)
    s = _jf_solver(case, dd)
    want = {al: W.jfnk_solve(f0, x, b, 1.0, -JK.GAMMA, y0, fdtype, d if pc == "diag" else None, WC.jfnk_lent(case) if case["kind"] else None,
                             case["rtol"], case["maxit"], True, case["restart"], num_cus, x_aligned=not xoff, y0_aligned=al, small_off=True)
            for al in (False, True)}
    s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA, y0=y0d)
    st, got = s.status(), yd.cpu().numpy()
    assert st == want[False][1] and HW._same(got, want[False][0])
    assert _intact(y0b, y0, 1) and _intact(xb, x, xoff) and _intact(yb)
    if not xoff:                                  # the order is visible: on a pair the same y0 gives other bits
        assert not HW._same(want[True][0], want[False][0])
        s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA, y0=_guarded(y0)[1])
        assert s.status() == want[True][1] and HW._same(yd.cpu().numpy(), want[True][0])


# ---- 5. the plain-C clients ------------------------------------------------------------------------------------------------------------------
def _client(tmp_path, name):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", name + ".c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_the_sparse_client_prints_what_the_python_path_computes(tmp_path):
    out = _client(tmp_path, "csc_warm_client")
    assert "csc warm: PASS" in out, out
    steps = [tuple(map(int, m)) for m in re.findall(r"step \d+: cold status (\d+) iterations (\d+), warm status (\d+) iterations (\d+)", out)]
    worst_c = float(re.search(r"max \|y_warm - y_cold\| = (\S+)", out).group(1))
    colptr, rowval, N, nz, u, rl = WC.client_sequence()
    s = fd.CscSolver((colptr, rowval, N), idx_base=0)
    s.set_options(WC.SEQ_RTOL, 500)
    nzd, ud = _guarded(nz)[1], _guarded(u)[1]
    cold, warm = _guarded(np.zeros(N))[1], _guarded(np.zeros(N))[1]
    mine, worst = [], 0.0
    for _step in range(WC.SEQ_STEPS):
        s.solve(nzd, ud, cold, 1.0, -WC.SEQ_GAMMA)
        c = s.status()
        s.solve(nzd, ud, warm, 1.0, -WC.SEQ_GAMMA, y0=ud)
        w = s.status()
        mine.append((c["flags"], c["iterations"], w["flags"], w["iterations"]))
        worst = max(worst, float((warm - cold).abs().max()))
        ud.copy_(cold)
    print(out, mine, worst)
    assert steps == mine and len(steps) == 4 and worst_c == worst


def test_the_matrix_free_client_prints_what_the_python_path_computes(tmp_path):
    out = _client(tmp_path, "jfnk_warm_client")
    assert "jfnk warm: PASS" in out, out
    calls = [(int(a), int(b), float(c)) for a, b, c in re.findall(r"call \d+: status (\d+) iterations (\d+) estimate (\S+)", out)]
    N, gamma = 20001, 0.3
    i = np.arange(N)
    x = 0.25 + 0.5 * (i % 7) / 7.0
    b = 1.0 - gamma * (-2.0 + (i > 0) + (i + 1 < N))
    f = fd.BuiltinF("tridiag", N)
    s = fd.JfnkSolver(N, "forward", 30)
    s.set_options(1e-6, 3)
    s.set_policy(True)
    s.set_lazy(f)
    xd, bd = _guarded(x)[1], _guarded(b)[1]
    yb, yd = _guarded(np.full(N, CANARY))
    mine = []
    while not mine or (mine[-1][0] == 1 and len(mine) < 50):
        s.solve(f, xd, bd, yd, 1.0, -gamma, y0=yd if mine else None)
        st = s.status()
        mine.append((st["flags"], st["iterations"], st["resid"]))
    print(out, mine)
    assert calls == mine and len(calls) >= 2 and calls[-1][0] == 0 and _intact(yb)
