"""The matrix-free trust-region consumer on the CPU: the numpy model (tests/jftr_model.py) against csc_tr_model.step with the stored
product plugged in (the factoring identity), its piece of the JVP's dot against jvp_model, the model against the stored Hessian of the
linear families, Steihaug's properties on the model's own steps, and the new entry points' argument errors at the ABI.

AGAINST THE STORED H.  On tridiag / lap5 the Jacobian is constant and symmetric, so B = lam I + beta J can be stored exactly (entries
beta * {-2, 1} / {-4, 1}) and handed to the stored recurrence: cg() with csc_tr_model's row product, dot_rows and k_tr_p's dots, which the
factoring identity shows to be csc_tr_model.step; the caller's m stands in for that model's |H_jj| + lam.  The matrix-free operator
differs from B by the quotient's rounding noise, about eps / eps_fd = 1.5e-8 relative (forward; the central step is larger and the noise
smaller), so with rtol = 1e-6 both recurrences take the same decisions as long as the stored one is not close to a decision: the test
checks that every comparison the stored run makes (||y + alpha p||_W against Delta, ||r|| against rtol ||g||) is at least 10 % away from
equality, and that |kappa| is at least 1 % of ||B|| p.p (a sign has no 10 % margin; this is six orders above the noise).  Then: the same exit kind, the same iteration
count, and ||y - y_stored|| / ||y_stored|| at most ALLOWED = ten times the largest value this file measures over STORED_CASES
(MEASURED below restates it; test_the_measured_value_is_current recomputes it), capped at 1e-4.  DESIGN.md 4.13 has both numbers.

PROPERTIES.  q(y) < 0 with q evaluated on the exact B in np.longdouble; | ||y||_W - Delta | <= 50 eps Delta on exits 1 and 2, the bound
tests/test_csctr_model_cpu.py derives for dots of kCsVecTile tiles (the cases here stay at or below kSmallN, where the pi dots are
k_tr_p's); ||y_k||_W increases along the iterates -- strictly over the first eight of an interior run and over all of a boundary run; late
in a converged interior run the increment falls below the operator's noise (1.5e-8 ||y||), where it may only not DEcrease by more."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as M
import csc_tr_model as TM
import jfnk_model as JM
import jftr_cases as K
import jftr_model as TR
import jvp_model as J
import test_csctr_model_cpu as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
INF = float("inf")
MEASURED = 1.8e-7          # the largest ||y - y_stored|| / ||y_stored|| over STORED_CASES: 1.73e-7 (tridiag 1025, forward, W = I, interior)
ALLOWED = min(10 * MEASURED, 1e-4)
MARGIN = 0.1
RTOL = 1e-6
NOISE = 1e-7               # several times eps / eps_fd = 1.5e-8: below this, relative to ||y||, the operator's asymmetry decides a sign


@pytest.fixture(scope="module", autouse=True)
def _the_library_has_the_consumer():
    """These tests need only numpy, yet they describe fd_jftr_*: a tree without those entry points has nothing the model is a model of.
    So the module asks the built library for them first and every test here fails where they are missing."""
    fd.lib.build()
    assert hasattr(fd.lib.load(), "fd_jftr_step_async") and hasattr(fd, "JfTrustRegion")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b)) or (np.all(np.isnan(a)) and np.all(np.isnan(b)))


# ---- the factoring identity -------------------------------------------------------------------------------------------------------------
def _stored_cg(rl, lam, kind, nz, g, radius, rtol, maxit, keep=False, trace=None, log=None, m=None):
    if m is None:
        m = TM.precond(rl, np.float64(lam), kind, nz)
        with np.errstate(all="ignore"):
            bad = kind == TM.NORM_DIAG and not np.all((np.abs(m) > 0.0) & (np.abs(m) < np.inf))
    else:
        bad = False
    lam64 = np.float64(lam)
    return TR.cg(lambda p: TM.row_sums(rl, nz, p) + lam64 * p, M.dot_rows, TR.pi_dots_vec, m, bad, g, radius, rtol, maxit, keep, trace, log)


@pytest.mark.parametrize("name,lam,kind,radius", H.ALL_STEPS[::2] + [("spd_long", 0.25, 1, "inf")])
def test_the_copy_is_csc_tr_models_step_with_the_stored_product(name, lam, kind, radius):
    colptr, rowval, nz, N, g, rl = H.case(name)
    want_y, want_r, wst, wtrace = H.model_step(name, lam, kind, radius)
    trace = []
    y, r, st = _stored_cg(rl, lam, kind, nz, g, H.radius_of(name, lam, kind, radius), H.RTOL, H.MAXIT, trace=trace)
    assert TM.same_status(st, wst) and _same(y, want_y) and _same(r, want_r)
    assert len(trace) == len(wtrace) and all(_same(a, b) for a, b in zip(trace, wtrace))


def test_the_copy_follows_csc_tr_models_failure_paths():
    colptr, rowval, nz, N, g, rl = H.case("spd")
    ic, ir, inz, iN, ig, il = H.case("indef")
    nz0 = nz.copy(); nz0[rl.diag[17]] = 0.0
    nzn = nz.copy(); nzn[5] = np.nan
    runs = [(rl, 0.0, 0, nz, g, INF, 3), (rl, 0.0, 1, nz0, g, INF, 50), (il, 0.0, 0, inz, ig, INF, 50), (il, 0.0, 1, inz, ig, 1e200, 50),
            (rl, 0.0, 1, nzn, g, INF, 50), (rl, 0.0, 1, nz, np.zeros(N), 1.0, 50)]
    for lists, lam, kind, vals, gg, radius, maxit in runs:
        for keep in (False, True):
            want = TM.step(lists, lam, radius, kind, vals, gg, H.RTOL, maxit, keep_unconverged=keep)
            got = _stored_cg(lists, lam, kind, vals, gg, radius, H.RTOL, maxit, keep)
            assert TM.same_status(got[2], want[2]) and _same(got[0], want[0]) and _same(got[1], want[1])


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1025, 16385, 16386, 70001])
def test_the_workgroups_sums_are_jvp_models(n):
    """wg_sums restates jvp_model.dot_large's loop up to the partials: k_jvp_eps's sum of them must give dot_large itself."""
    rng = np.random.default_rng(n)
    x, p = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    for paired in (False, True):
        for cus in (4, 256):
            parts = TR.wg_sums(x * p, paired, cus)
            assert parts.size == J.grid(n, cus)
            got = J._tree_waves(J._strided(np.zeros(J.BLOCK), parts))
            assert _bits(got) == _bits(J.dot_large(x, p, paired, cus))


def test_the_ascending_sum_is_another_order_than_k_tr_ps():
    differ = 0
    for seed in range(8):
        t = np.random.default_rng(seed).uniform(0.5, 1, 300001) ** 2
        differ += int(TR.ascending(TR.wg_sums(t, True, 256)) != M.dot_vec(t, np.ones(t.size)))
    assert differ >= 1


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_check_their_arguments():
    fd.lib.build()
    L = fd.lib.load()
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    shim = open(os.path.join(ROOT, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    names = ("create", "destroy", "set_options", "set_policy", "set_steps", "set_lazy_f", "set_diagonal", "apply_async", "step_async", "status",
             "counts")
    for n in names:
        assert re.search(r"^int fd_jftr_%s\(" % n, hdr, re.M), n
        assert hasattr(L, "fd_jftr_" + n) and "fd_jftr_" + n in fd.lib.EXPORTS
        assert not hasattr(L, "fd32_jftr_" + n) and "fd_jftr_" + n not in fd.lib.TYPED          # Float64 only
        assert ":fd_jftr_%s," % n in shim, n
    ARG, SHAPE, UNSUPPORTED = 1, 2, 3
    err = lambda: L.fd_last_error().decode()          # noqa: E731
    h = C.c_void_p()
    assert L.fd_jftr_create(None, 10, 0, C.byref(h)) == ARG and "NULL" in err()
    assert L.fd_jftr_destroy(None) == 0
    assert L.fd_jftr_set_options(None, 1e-6, 10) == ARG and "tr is NULL" in err()
    assert L.fd_jftr_set_policy(None, 1) == ARG
    assert L.fd_jftr_set_steps(None, -1.0, -1.0, 1.0) == ARG
    assert L.fd_jftr_set_lazy_f(None, fd.lib.F_LAUNCH_LAZY_JVP(), 0) == ARG
    assert L.fd_jftr_set_diagonal(None, None) == ARG
    assert L.fd_jftr_apply_async(None, 0.0, 1.0, fd.lib.F_LAUNCH(), None, None, None, None, None) == ARG and "NULL" in err()
    assert L.fd_jftr_step_async(None, 0.0, 1.0, 1.0, fd.lib.F_LAUNCH(), None, None, None, None, None, None) == ARG and "NULL" in err()
    assert L.fd_jftr_status(None, None, None, None, None, None, None, None) == ARG
    assert L.fd_jftr_counts(None, None, None) == ARG
    # the range checks come before the device is touched (fd_jftr_create keeps them ahead of its first use of ctx, and says so):
    # a context that is never dereferenced stands in for one
    fake = C.c_void_p(8)
    assert L.fd_jftr_create(fake, 0, 0, C.byref(h)) == SHAPE and "N = 0" in err()
    assert L.fd_jftr_create(fake, 2 ** 31 - 1024, 0, C.byref(h)) == SHAPE
    assert L.fd_jftr_create(fake, 10, 2, C.byref(h)) == UNSUPPORTED and "complex-mode" in err()
    assert L.fd_jftr_create(fake, 10, 7, C.byref(h)) == UNSUPPORTED
    assert h.value is None
    # ... and those of a step and of an application before anything is enqueued: a handle, a launcher and arrays that are never touched
    @fd.lib.F_LAUNCH
    def never(*_a):          # pragma: no cover
        raise AssertionError("the launcher must not run")
    a, b, c = (C.c_void_p(64 * k) for k in (1, 2, 3))
    step = lambda lam, beta, radius, x=a, g=b, y=c, r=None, f=never: L.fd_jftr_step_async(fake, lam, beta, radius, f, None, x, None, g, y, r)   # noqa: E731
    assert step(-0.5, 1.0, 1.0) == ARG and "lambda = -0.5" in err()
    assert step(INF, 1.0, 1.0) == ARG and step(float("nan"), 1.0, 1.0) == ARG
    assert step(0.0, 0.0, 1.0) == ARG and "beta = 0" in err()
    assert step(0.0, INF, 1.0) == ARG and step(0.0, float("nan"), 1.0) == ARG
    assert step(0.0, 1.0, 0.0) == ARG and "radius = 0" in err()
    assert step(0.0, 1.0, -1.0) == ARG and step(0.0, 1.0, float("nan")) == ARG
    assert step(0.0, 1.0, 1.0, x=None) == ARG and step(0.0, 1.0, 1.0, g=None) == ARG and step(0.0, 1.0, 1.0, y=None) == ARG
    assert step(0.0, 1.0, 1.0, f=fd.lib.F_LAUNCH()) == ARG
    assert step(0.0, 1.0, 1.0, y=a) == ARG and "must not be x" in err() and step(0.0, 1.0, 1.0, r=a) == ARG
    app = lambda lam, beta, x=a, v=b, w=c: L.fd_jftr_apply_async(fake, lam, beta, never, None, x, None, v, w)   # noqa: E731
    assert app(-1.0, 1.0) == ARG and app(0.0, 0.0) == ARG and app(0.0, 1.0, w=b) == ARG and "must not be v or x" in err()
    assert app(0.0, 1.0, w=a) == ARG and app(0.0, 1.0, v=None) == ARG


# ---- against the stored H of the linear families --------------------------------------------------------------------------------------------
def _stored_b(family, prm, lam, beta):
    """(RowLists, nz) of beta J, J the constant Jacobian of tridiag / lap5, and the extreme |eigenvalue| bound of lam I + beta J."""
    N = K.size_of(family, prm)
    Jd = JM.jacobian_dense(family, prm, np.zeros(N))
    cols, rows = np.nonzero(Jd.T)                              # by column, rows ascending
    colptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=N))]).astype(np.int64)
    return TM.RowLists(colptr, rows.astype(np.int64), N), (beta * Jd.T[cols, rows]).astype(np.float64), Jd


# (family, prm, fdtype, m set, (lam, beta, radius)); a relative radius is a multiple of the STORED interior step's ||y*||_W.  The factors
# 0.7 (two iterations), 0.4, 0.1 and 1e-3 (one) are chosen for the margin: with 0.5 the tridiagonal runs come within 1 % of the boundary
# test, with 0.6 the 5-point ones
STORED_MODELS = K.INTERIOR + tuple((0.5, -1.0, ("rel", f)) for f in (0.7, 0.4, 0.1, 1e-3)) + K.NEGATIVE + K.UNBOUNDED
STORED_EXIT = dict([(e, 0) for e in K.INTERIOR] + [(e, 2) for e in K.NEGATIVE] + [(e, 3) for e in K.UNBOUNDED])
STORED_CASES = [(fam, prm, fdt, diag, mdl)
                for fam, prm in (("tridiag", (255,)), ("tridiag", (1025,)), ("lap5", (7, 9)), ("lap5", (16, 15)))
                for fdt, diag in (("forward", False), ("central", True), ("forward", True))
                for mdl in STORED_MODELS]


def _stored_run(fam, prm, diag, mdl):
    lam, beta, radius = mdl
    f, x, g, m0 = K.system(fam, prm)
    rl, nz, Jd = _stored_b(fam, prm, lam, beta)
    m = m0 if diag else np.ones(x.size)
    star = _stored_cg(rl, lam, 0, nz, g, INF, RTOL, K.MAXIT, keep=True, m=m)[2]["step_norm"]
    delta = INF if radius == "inf" else (radius[1] * star if isinstance(radius, tuple) else float(radius))
    log, trace = [], []
    y, r, st = _stored_cg(rl, lam, 0, nz, g, delta, RTOL, K.MAXIT, keep=True, trace=trace, log=log, m=m)
    return f, x, g, m, delta, (y, r, st), log, trace, Jd


_measured = {}


def _measure(case):
    """||y - y_stored|| / ||y_stored|| of a case (0.0 on exit 3, which has no step), after the checks of the module docstring."""
    if case in _measured:
        return _measured[case]
    fam, prm, fdt, diag, mdl = case
    lam, beta, radius = mdl
    f, x, g, m, delta, (ys, rs, sts), log, _trace, Jd = _stored_run(fam, prm, diag, mdl)
    scale = max(abs(lam - 8.0 * beta), abs(lam))          # ||B|| is at most this
    for k, e in enumerate(log):
        if e["reach"] is not None and np.isfinite(e["delta2"]):
            assert abs(np.sqrt(e["reach"]) / np.sqrt(e["delta2"]) - 1.0) >= MARGIN, (case, k, e)
        assert abs(np.sqrt(e["rho"]) / np.sqrt(e["tol2"]) - 1.0) >= MARGIN, (case, k, e)
        assert abs(e["kappa"]) >= 0.01 * scale * e["pp"], (case, k, e)
    y, r, st = TR.step(f, x, g, lam, beta, delta, fdt, m if diag else None, RTOL, K.MAXIT, keep_unconverged=True)
    assert (st["exit"], st["iterations"], st["flags"]) == (sts["exit"], sts["iterations"], sts["flags"]), (case, st, sts)
    assert st["exit"] == STORED_EXIT.get(mdl, 1)
    if st["exit"] == 3:
        assert st["iterations"] == 0 and not y.any()
        err = 0.0
    else:
        err = float(np.linalg.norm(y - ys) / np.linalg.norm(ys))
    _measured[case] = err
    return err


@pytest.mark.parametrize("case", STORED_CASES, ids=lambda c: "-".join(map(str, c[:4])) + "-" + "_".join(map(str, c[4])))
def test_the_model_agrees_with_the_stored_hessian(case):
    err = _measure(case)
    print("||y - y_stored|| / ||y_stored|| = %.3e (allowed %.3e)" % (err, ALLOWED))
    assert err <= ALLOWED


def test_the_measured_value_is_current():
    worst = max(_measure(c) for c in STORED_CASES)
    print("largest ||y - y_stored|| / ||y_stored|| = %.3e, MEASURED = %.3e, ALLOWED = %.3e" % (worst, MEASURED, ALLOWED))
    assert ALLOWED <= 1e-4 and MEASURED / 2 <= worst <= MEASURED


# ---- properties of the model's own steps ----------------------------------------------------------------------------------------------------
PROPERTY_CASES = [c for c in K.CASES + K.EXITS if not c["family"].endswith("_nl") and K.size_of(c["family"], c["prm"]) <= J.SMALL_N]


@pytest.mark.parametrize("case", PROPERTY_CASES, ids=lambda c: c["id"])
def test_steihaugs_properties_on_the_models_steps(case):
    f, x, g, m0 = K.operands(case)
    N = x.size
    m = (m0 if case["diag"] else np.ones(N)).astype(np.longdouble)
    B = (case["lam"] * np.eye(N) + case["beta"] * JM.jacobian_dense(case["family"], case["prm"], x)).astype(np.longdouble) if N <= 2100 else None
    trace = []
    y, r, st = K.model(case, trace=trace)
    delta = K.radius_of(case)
    norm_w = lambda v: np.sqrt((m * v.astype(np.longdouble) ** 2).sum())          # noqa: E731
    assert st["iterations"] == len(trace)
    if st["exit"] == 3 or st["iterations"] == 0:
        return
    if B is not None:
        yl = y.astype(np.longdouble)
        q = (g * yl).sum() + (yl * (B @ yl)).sum() / 2
        assert q < 0
    if st["exit"] in (1, 2):
        assert st["flags"] == 0
        assert abs(norm_w(y) - delta) <= H.BOUNDARY_C * EPS * delta and abs(st["step_norm"] - delta) <= H.BOUNDARY_C * EPS * delta
    else:
        assert st["step_norm"] < delta
    norms = [np.longdouble(0)] + [norm_w(v) for v in trace]
    head = norms[:9] if st["exit"] == 0 else norms
    assert all(b > a for a, b in zip(head, head[1:]))
    assert all(b - a > -NOISE * b for a, b in zip(norms, norms[1:]))


def test_the_cpu_cases_reach_every_exit_and_route():
    assert {STORED_EXIT.get(c[4], 1) for c in STORED_CASES} == {0, 1, 2, 3}
    assert {K.model(c)[2]["exit"] for c in PROPERTY_CASES} == {0, 1, 2, 3}
    for c in K.EXITS:
        assert K.model(c)[2]["exit"] == K.WANT_EXIT[(c["lam"], c["beta"], c["radius"])], c["id"]


def test_failures_of_the_model():
    c = K._case("tridiag", (257,), "forward", diag=True, model=K.INTERIOR[0])
    f, x, g, m = K.operands(c)
    y, r, st = K.model(c, g=np.zeros(x.size))
    assert st == {"flags": 0, "exit": 0, "iterations": 0, "resid": 0.0, "g_norm": 0.0, "step_norm": 0.0, "pred": 0.0} and not y.any()
    for bad in (0.0, -1.0, np.nan, np.inf):
        mm = m.copy(); mm[11] = bad
        y, r, st = K.model(c, m=mm, keep=False)
        assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y)) and np.all(np.isnan(r)), bad
    xx = x.copy(); xx[5] = np.nan
    cnt = {}
    y, r, st = K.model(c, x=xx, counts=cnt)
    assert st["flags"] == 2 and st["iterations"] == 0 and cnt["applications"] == 1 and not y.any()
    y, r, st = K.model(c, maxit=3, keep=False)
    assert st["flags"] == 1 and st["iterations"] == 3 and np.all(np.isnan(y))
    y, r, st = K.model(c, maxit=3)
    assert st["flags"] == 1 and np.all(np.isfinite(y)) and st["pred"] > 0
