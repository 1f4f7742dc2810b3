"""The trust-region consumer on the CPU: the numpy model of csrc/fdjac_csctr.hip (tests/csc_tr_model.py) against SciPy, against its own
mathematics in extended precision and against a plain dense Steihaug-CG, its failure paths -- and the new symbols at the ABI.

INTERIOR EXITS.  A = H + lambda I is symmetric positive definite with smallest eigenvalue lambda_min, and r(y) = g + A y.  For any two
vectors y, z:  y - z = A^-1 (r(y) - r(z)), hence
    ||y - y_ref||_2 <= (||r(y)||_2 + ||r(y_ref)||_2) / lambda_min,
with r evaluated in np.longdouble.  So that the bound cannot hide a failure its right-hand side must itself be at most 1e-6 ||y_ref||_2,
the project's relative contract; the diagonals of `spd` and `spd_long` are chosen so that the reference alone meets this (asserted).

THE PRODUCT.  Each result is a sum of n rounded products in SOME order plus lambda v_r; whatever the order, |computed - exact| <=
(n + 1) eps sum|terms| to first order.  Model and SciPy each stay within that, so they differ by at most 2 (n + 2) eps sum|terms|.

BOUNDARY EXITS.  The step to the boundary is y' = y + tau p with tau the positive root of pi_yy + 2 tau pi_yp + tau^2 pi_pp = Delta^2.
Write k = D + 2 for a weighted dot of non-negative terms (two roundings per term and a summation tree of depth D = 4 + 9 + ceil(tiles / 256)
+ 9: four terms per thread, block_sum, the tiles' sums strided and block_sum again; D = 23 here).  To first order:
  - the computed pi_yy, pi_pp are within k eps of the true sums A = ||y||_W^2, C = ||p||_W^2, and pi_yp within k eps sqrt(A C) of B = y.Wp
    (Cauchy-Schwarz), so at the exact root of the COMPUTED quadratic the TRUE ||y + tau p||_W^2 misses Delta^2 by at most
    k eps (sqrt(A) + tau sqrt(C))^2 <= 2 k eps Delta^2 -- B >= 0 in Steihaug's method, hence A + tau^2 C <= Delta^2 -- i.e. the norm by
    k eps Delta;
  - tau itself is computed with at most t = 8 roundings, none of them a cancellation (pi_yp >= 0, Delta^2 > pi_yy), and
    d||y + tau p||_W^2 / d tau = 2 (B + tau C) with tau B + tau^2 C <= Delta^2: another t eps Delta on the norm;
  - the element-wise update rounds tau p_j and the sum: at most eps (tau ||p||_W + ||y'||_W) <= 2.5 eps Delta;
  - ||y'||_W as the status reports it carries its own dot (k / 2 eps Delta on the norm) and a square root (eps Delta).
So | ||y'||_W - Delta | <= c eps Delta with c = 1.5 k + t + 4 = 49.5 for k = 25: BOUNDARY_C = 50.

PRED.  pred = -1/2 sum y_j (g_j + r_j) is one dot of N terms (one addition, one product per term, the tree of depth D, the exact halving):
|pred - exact dot| <= (D + 3) eps 1/2 sum |y_j| |g_j + r_j|.  -q(y) = -1/2 y.(g + r_true) with r_true = g + A y, so pred misses -q(y) by
that and by at most 1/2 ||y||_2 ||r - r_true||_2, the drift of the recurred model gradient (itself held to 1e-12 ||g||_2, the contract the
neighbouring consumers' tests hold their recurred residuals to)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_tr_model as TM

try:                       # SciPy is the reference of the product and of the interior exits; everything else must run without it
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
except ImportError:        # pragma: no cover
    sp = spla = None
needs_scipy = pytest.mark.skipif(sp is None, reason="needs SciPy")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, MAXIT = 1e-10, 500
EPS = np.finfo(float).eps
BOUNDARY_C = 50.0
INF = float("inf")
NEG_RADIUS = 100.0         # `indef`: large enough that the iteration meets the negative curvature before the boundary
_cache = {}

# (case, lambda, norm kind, radius): the radius is "inf", an absolute number (`indef`), or ("rel", f): f ||y*||_W with y* the model's own
# interior solution for that (case, lambda, kind)
INTERIOR = [(name, lam, kind, radius) for name in ("spd", "spd_long") for lam, kind in ((0.0, 0), (0.0, 1), (0.25, 1))
            for radius in ("inf", ("rel", 2.0))]
BOUNDARY = [("spd", 0.0, kind, ("rel", f)) for kind in (0, 1) for f in (0.5, 0.1, 1e-3, 0.97)]      # (0.97: several iterations inside first)
NEGATIVE = [("indef", 0.0, 0, NEG_RADIUS), ("indef", 0.0, 1, NEG_RADIUS), ("indef", 0.25, 1, NEG_RADIUS)]
ALL_STEPS = INTERIOR + BOUNDARY + NEGATIVE


def case(name):
    """(colptr, rowval, nz, N, g, lists) of a named case, built once."""
    if name not in _cache:
        colptr, rowval, nz, N = TM.named_case(name)
        g = np.random.default_rng(1).uniform(-1.0, 1.0, N)
        _cache[name] = (colptr, rowval, nz, N, g, TM.RowLists(colptr, rowval, N))
    return _cache[name]


def radius_of(name, lam, kind, radius):
    if radius == "inf":
        return INF
    if isinstance(radius, tuple):
        return radius[1] * model_step(name, lam, kind, "inf")[2]["step_norm"]
    return float(radius)


def model_step(name, lam, kind, radius):
    """(y, r_out, status, iterates) of the model, computed once per case and left unchanged."""
    key = ("step", name, lam, kind, radius)
    if key not in _cache:
        colptr, rowval, nz, N, g, rl = case(name)
        trace = []
        y, r, st = TM.step(rl, lam, radius_of(name, lam, kind, radius), kind, nz, g, RTOL, MAXIT, trace=trace)
        _cache[key] = (y, r, st, trace)
    return _cache[key]


class Exact:
    """A = H + lambda I, g and the weights in np.longdouble: r(y), q(y), ||y||_W."""

    def __init__(self, name, lam, kind):
        colptr, rowval, nz, N, g, rl = case(name)
        self.N = N
        self.rows = rowval
        self.cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
        self.vals = nz.astype(np.longdouble)
        self.lam = np.longdouble(lam)
        self.g = g.astype(np.longdouble)
        self.w = TM.precond(rl, lam, kind, nz).astype(np.longdouble)

    def Ax(self, y):
        y = np.asarray(y, dtype=np.longdouble)
        out = np.zeros(self.N, dtype=np.longdouble)
        np.add.at(out, self.rows, self.vals * y[self.cols])
        return out + self.lam * y

    def r(self, y):
        return self.g + self.Ax(y)

    def q(self, y):
        y = np.asarray(y, dtype=np.longdouble)
        return (self.g * y).sum() + (y * self.Ax(y)).sum() / 2

    def norm_w(self, y):
        y = np.asarray(y, dtype=np.longdouble)
        return np.sqrt((self.w * y * y).sum())

    def cauchy(self, radius):
        """The minimiser of q along -W^-1 g within the region."""
        p = -self.g / self.w
        kappa, gamma, pn = (p * self.Ax(p)).sum(), (self.g * self.g / self.w).sum(), self.norm_w(p)
        t = radius / pn if kappa <= 0 else min(gamma / kappa, radius / pn)
        return t * p


def exact(name, lam, kind):
    key = ("exact", name, lam, kind)
    if key not in _cache:
        _cache[key] = Exact(name, lam, kind)
    return _cache[key]


def reference(name, lam):
    """(A, lambda_min, y_ref) by a sparse direct solve, built once per case."""
    key = ("ref", name, lam)
    if key not in _cache:
        colptr, rowval, nz, N, g, rl = case(name)
        A = (sp.csc_matrix((nz, rowval, colptr), shape=(N, N)) + lam * sp.identity(N)).tocsc()
        lmin = float(spla.eigsh(A, k=1, sigma=0, which="LM", return_eigenvectors=False)[0])
        _cache[key] = (A, lmin, spla.spsolve(A, -g))
    return _cache[key]


def derived_bound(name, lam, y):
    """(error, bound, bound / ||y_ref||) of the module docstring for the vector y."""
    A, lmin, y_ref = reference(name, lam)
    E = exact(name, lam, 0)
    assert lmin > 0
    res = lambda v: float(np.sqrt((E.r(v) ** 2).sum()))      # noqa: E731
    err = np.linalg.norm(np.asarray(y, dtype=np.float64) - y_ref)
    bound = (res(y) + res(y_ref)) / lmin
    return err, bound, bound / np.linalg.norm(y_ref)


def tree_depth(N):
    return 4 + 9 + (((N + 1023) // 1024 + 255) // 256) + 9


def check_boundary_step(name, lam, kind, radius, y, r, st):
    """What a boundary exit (1 or 2) must satisfy, for the model's y or the device's: module docstring."""
    E = exact(name, lam, kind)
    delta = radius_of(name, lam, kind, radius)
    colptr, rowval, nz, N, g, rl = case(name)
    assert st["flags"] == 0 and np.all(np.isfinite(y))
    nw = E.norm_w(y)
    print("    | ||y||_W - Delta | = %.2f eps Delta (allowed %.0f); status %.2f eps" % (abs(nw - delta) / (EPS * delta), BOUNDARY_C,
                                                                                        abs(st["step_norm"] - delta) / (EPS * delta)))
    assert abs(nw - delta) <= BOUNDARY_C * EPS * delta
    assert abs(st["step_norm"] - delta) <= BOUNDARY_C * EPS * delta
    qy, yc = E.q(y), E.cauchy(delta)
    slack = BOUNDARY_C * EPS * float((np.abs(yc) * (np.abs(E.g) + np.abs(E.Ax(np.abs(yc))))).sum())      # |grad q| . |dy|, |dy| <= c eps |y|
    print("    q(y) = %.6e, q(Cauchy) = %.6e" % (float(qy), float(E.q(yc))))
    assert qy < 0 and qy <= E.q(yc) + slack
    check_pred(name, lam, kind, y, r, st)


def check_pred(name, lam, kind, y, r, st):
    E = exact(name, lam, kind)
    colptr, rowval, nz, N, g, rl = case(name)
    yl, rl_ = y.astype(np.longdouble), r.astype(np.longdouble)
    drift = float(np.sqrt(((rl_ - E.r(y)) ** 2).sum()))
    assert drift <= 1e-12 * np.linalg.norm(g)
    dot_bound = (tree_depth(N) + 3) * EPS * 0.5 * float((np.abs(yl) * np.abs(E.g + rl_)).sum())
    print("    pred + q(y) = %.3e (dot bound %.3e, drift term %.3e)" % (float(st["pred"] + E.q(y)), dot_bound, 0.5 * np.linalg.norm(y) * drift))
    assert abs(st["pred"] + (yl * (E.g + rl_)).sum() / 2) <= dot_bound
    assert abs(st["pred"] + E.q(y)) <= dot_bound + 0.5 * np.linalg.norm(y) * drift


def test_named_cases_are_what_they_claim():
    colptr, rowval, nz, N, g, rl = case("spd")
    assert N == 3000 and (N + 255) // 256 == 12 and (N + 1023) // 1024 == 3 and rl.nlong == 0
    assert np.all(rl.diag >= 0) and np.all(nz[rl.diag] >= TM.abs_row_sums(**TM.BAND) + 1.0)      # strictly dominant, positive
    for name in ("spd", "spd_long", "indef"):             # symmetric bit for bit: the transposed pattern holds the same values
        cp, rv, vals, n, _g, lists = case(name)
        assert np.array_equal(lists.row_ptr, cp) and np.array_equal(lists.row_col, rv) and np.array_equal(vals[lists.row_slot], vals)
    ll = case("spd_long")[5]
    assert ll.nlong == 3 and [int(ll.lens[i]) for i in (100, 1500, 2999)] == [33, 300, 2500] and sorted(ll.lens)[-4] <= 32
    ic, ir, inz, iN, ig, il = case("indef")
    flipped = inz[il.diag][3::10]
    assert flipped.size == 300 and np.all(flipped <= -1.0)        # e_j.H e_j = H_jj < 0: lambda_min <= H_jj < 0
    assert np.array_equal(np.delete(inz, il.diag[3::10]), np.delete(nz, rl.diag[3::10]))
    if sp is not None:
        Hs = sp.csc_matrix((inz, ir, ic), shape=(iN, iN))
        lmin = float(spla.eigsh(Hs, k=1, which="SA", return_eigenvectors=False)[0])
        print("indef: lambda_min = %.3f" % lmin)
        assert lmin < 0


@needs_scipy
@pytest.mark.parametrize("name", ["spd_long", "indef", "tiny"])
def test_product_equals_scipy_to_the_derived_bound(name):
    pats = [TM.tiny_case(n) for n in (1, 2, 3)] if name == "tiny" else [case(name)[:4]]
    rng = np.random.default_rng(9)
    for colptr, rowval, nz, N in pats:
        rl = TM.RowLists(colptr, rowval, N)
        H = sp.csc_matrix((nz, rowval, colptr), shape=(N, N))
        for lam in (0.0, 0.7):
            v = rng.uniform(-1, 1, N)
            got = TM.matvec(rl, lam, nz, v)
            mag = abs(H) @ np.abs(v) + lam * np.abs(v)
            assert got.shape == (N,)
            assert np.all(np.abs(got - (H @ v + lam * v)) <= 2 * (int(rl.lens.max()) + 2) * EPS * mag)


@needs_scipy
@pytest.mark.parametrize("name,lam,kind,radius", INTERIOR)
def test_interior_exits_meet_the_derived_bound(name, lam, kind, radius):
    colptr, rowval, nz, N, g, rl = case(name)
    y, r, st, trace = model_step(name, lam, kind, radius)
    print("%s lam %g kind %d radius %s: %s" % (name, lam, kind, radius, st))
    assert st["flags"] == 0 and st["exit"] == 0 and 1 <= st["iterations"] < MAXIT and st["resid"] <= RTOL * st["g_norm"]
    assert st["step_norm"] < radius_of(name, lam, kind, radius)
    A, lmin, y_ref = reference(name, lam)
    ref_alone = 2 * float(np.sqrt((exact(name, lam, 0).r(y_ref) ** 2).sum())) / lmin
    assert ref_alone <= 1e-6 * np.linalg.norm(y_ref)             # the reference alone meets the contract
    err, bound, rel = derived_bound(name, lam, y)
    print("    lambda_min %.3f error %.3e bound %.3e = %.3e ||y_ref||" % (lmin, err, bound, rel))
    assert rel <= 1e-6
    assert err <= bound
    check_pred(name, lam, kind, y, r, st)
    if radius != "inf":                                          # a region that holds y* changes nothing
        y2, r2, st2, _ = model_step(name, lam, kind, "inf")
        assert np.array_equal(y, y2) and np.array_equal(r, r2) and TM.same_status(st, st2)


@pytest.mark.parametrize("name,lam,kind,radius", BOUNDARY + NEGATIVE)
def test_boundary_and_negative_curvature_exits(name, lam, kind, radius):
    y, r, st, trace = model_step(name, lam, kind, radius)
    print("%s lam %g kind %d radius %s: %s" % (name, lam, kind, radius, st))
    assert st["exit"] == (TM.EXIT_NEGATIVE if name == "indef" else TM.EXIT_BOUNDARY)
    assert st["iterations"] == len(trace) >= 1
    check_boundary_step(name, lam, kind, radius, y, r, st)
    # Steihaug's monotonicity along the iterates: ||y_k||_W increases, q(y_k) decreases
    E = exact(name, lam, kind)
    norms = [np.longdouble(0)] + [E.norm_w(v) for v in trace]
    qs = [np.longdouble(0)] + [E.q(v) for v in trace]
    assert all(b > a for a, b in zip(norms, norms[1:])) and all(b < a for a, b in zip(qs, qs[1:]))


def test_monotonicity_along_a_long_run():
    """The same property over the first iterations of an interior run (while the decrease of q still exceeds np.longdouble's
    resolution of q itself), so that it is tested on more than the one or two iterates of a boundary exit."""
    for kind in (0, 1):
        y, r, st, trace = model_step("spd", 0.0, kind, "inf")
        E = exact("spd", 0.0, kind)
        head = trace[:8]
        norms = [np.longdouble(0)] + [E.norm_w(v) for v in head]
        qs = [np.longdouble(0)] + [E.q(v) for v in head]
        assert len(head) == 8 and all(b > a for a, b in zip(norms, norms[1:])) and all(b < a for a, b in zip(qs, qs[1:]))


# ---- an independent restatement: dense, no prescribed orders -----------------------------------------------------------------------------
DENSE_BAND = dict(N=400, half=40, per_col=4, seed=11)
DENSE_LONG = {100: 33, 399: 300}
DENSE_TOL = 4.7e-15        # ten times the largest difference measured (4.61e-16), and far below the cap of 1e-6


def dense_case(name):
    long = DENSE_LONG if name == "spd_long" else None
    diag = TM.abs_row_sums(long=long, **DENSE_BAND) + 1.0 + np.random.default_rng(5).uniform(0.0, 1.0, DENSE_BAND["N"])
    if name == "indef":
        diag[3::10] = -diag[3::10]
    colptr, rowval, nz, N = TM.sym_band(diag=diag, long=long, **DENSE_BAND)
    A = np.zeros((N, N))
    A[rowval, np.repeat(np.arange(N), np.diff(colptr))] = nz
    return colptr, rowval, nz, N, A, np.random.default_rng(1).uniform(-1.0, 1.0, N)


def dense_steihaug(A, g, radius, w, rtol, maxit):
    """Steihaug-Toint CG as the textbook states it (Conn, Gould, Toint, Algorithm 7.5.1), preconditioned by diag(w); numpy's own sums."""
    y, r = np.zeros_like(g), g.copy()
    z = r / w
    p = -z
    gamma, tol = r @ z, rtol * np.sqrt(g @ g)
    for it in range(1, maxit + 1):
        q = A @ p
        kappa = p @ q
        yy, yp, pp = (w * y) @ y, (w * y) @ p, (w * p) @ p
        to_boundary = (-yp + np.sqrt(yp * yp + pp * (radius * radius - yy))) / pp if np.isfinite(radius) else np.inf
        if kappa <= 0:
            if not np.isfinite(radius):
                return y, 3, it - 1
            return y + to_boundary * p, 2, it
        alpha = gamma / kappa
        if alpha >= to_boundary:
            return y + to_boundary * p, 1, it
        y, r = y + alpha * p, r + alpha * q
        if np.sqrt(r @ r) <= tol:
            return y, 0, it
        z = r / w
        gamma, beta = r @ z, (r @ z) / gamma
        p = -z + beta * p
    raise AssertionError("the iterations ran out")


def dense_runs():
    for name in ("spd", "spd_long", "indef"):
        for lam, kind in ((0.0, 0), (0.0, 1), (0.25, 1)):
            radii = (INF, NEG_RADIUS) if name == "indef" else (INF, ("rel", 2.0), ("rel", 0.5), ("rel", 0.1), ("rel", 1e-3))
            for radius in radii:
                yield name, lam, kind, radius


def test_model_agrees_with_a_plain_dense_steihaug_cg():
    worst = 0.0
    for name, lam, kind, radius in dense_runs():
        colptr, rowval, nz, N, A, g = dense_case(name) if ("dense", name) not in _cache else _cache[("dense", name)]
        _cache[("dense", name)] = (colptr, rowval, nz, N, A, g)
        rl = TM.RowLists(colptr, rowval, N)
        if isinstance(radius, tuple):
            radius = radius[1] * TM.step(rl, lam, INF, kind, nz, g, RTOL, MAXIT)[2]["step_norm"]
        y, r, st = TM.step(rl, lam, radius, kind, nz, g, RTOL, MAXIT, keep_unconverged=True)
        w = TM.precond(rl, lam, kind, nz)
        yd, exit_d, it_d = dense_steihaug(A + lam * np.eye(N), g, radius, w, RTOL, MAXIT)
        diff = np.linalg.norm(y - yd) / np.linalg.norm(yd)
        worst = max(worst, diff)
        print("%s lam %g kind %d radius %.4g: exit %d (dense %d) iterations %d (dense %d) |y - y_dense| / |y_dense| = %.3e"
              % (name, lam, kind, radius, st["exit"], exit_d, st["iterations"], it_d, diff))
        assert (st["exit"], st["iterations"]) == (exit_d, it_d)
        assert diff <= DENSE_TOL
    print("largest difference %.3e" % worst)


# ---- failure paths and edges ---------------------------------------------------------------------------------------------------------------
def without_diagonal_entry(colptr, rowval, nz, j, rl):
    """The same matrix with the entry (j, j) removed from the pattern."""
    s = int(rl.diag[j])
    cp = colptr.copy()
    cp[j + 1:] -= 1
    return cp, np.delete(rowval, s), np.delete(nz, s)


def test_model_failure_paths_and_edge_cases():
    colptr, rowval, nz, N, g, rl = case("spd")
    # the iterations run out
    y3, r3, st3 = TM.step(rl, 0.0, INF, 0, nz, g, RTOL, 3)
    assert st3["flags"] == 1 and st3["exit"] == 0 and st3["iterations"] == 3 and np.all(np.isnan(y3)) and np.all(np.isnan(r3))
    y3k, r3k, st3k = TM.step(rl, 0.0, INF, 0, nz, g, RTOL, 3, keep_unconverged=True)
    assert TM.same_status(st3k, st3) and np.all(np.isfinite(y3k)) and np.all(np.isfinite(r3k)) and st3["step_norm"] > 0 and st3["pred"] > 0
    # a zero diagonal with the diagonal norm: the value, and the entry that is not stored
    nz0 = nz.copy(); nz0[rl.diag[17]] = 0.0
    cp1, rv1, nz1 = without_diagonal_entry(colptr, rowval, nz, 17, rl)
    rl1 = TM.RowLists(cp1, rv1, N)
    assert rl1.diag[17] == -1 and rl1.nnz == rl.nnz - 1
    for lists, vals in ((rl, nz0), (rl1, nz1)):
        y, r, st = TM.step(lists, 0.0, INF, 1, vals, g)
        assert st["flags"] == 2 and st["iterations"] == 0 and st["exit"] == 0 and np.all(np.isnan(y)) and np.all(np.isnan(r))
        yk, rk, stk = TM.step(lists, 0.0, INF, 1, vals, g, keep_unconverged=True)
        assert stk["flags"] == 2 and np.array_equal(yk, np.zeros(N)) and np.array_equal(rk, g)
        for lam, kind in ((0.5, 1), (0.0, 0)):                   # lambda lifts it; the identity norm never divides by it
            y, r, st = TM.step(lists, lam, 1.0, kind, vals, g)
            assert st["flags"] == 0 and st["exit"] == 1
    # negative curvature and no boundary
    ic, ir, inz, iN, ig, il = case("indef")
    for kind in (0, 1):
        y, r, st = TM.step(il, 0.0, INF, kind, inz, ig)
        assert st["flags"] == 2 and st["exit"] == 3 and np.all(np.isnan(y)) and np.all(np.isnan(r))
        yk, rk, stk = TM.step(il, 0.0, INF, kind, inz, ig, keep_unconverged=True)
        assert TM.same_status(stk, st) and np.all(np.isfinite(yk)) and st["step_norm"] > 0
        y, r, st = TM.step(il, 0.0, 1e200, kind, inz, ig)        # Delta^2 = +Inf in Float64: no boundary either
        assert st["flags"] == 2 and st["exit"] == 3
    # a NaN in H is a breakdown, not a hang
    nzn = nz.copy(); nzn[5] = np.nan
    for kind in (0, 1):
        y, r, st = TM.step(rl, 0.0, INF, kind, nzn, g)
        assert st["flags"] == 2 and st["exit"] == 0 and np.all(np.isnan(y)) and np.all(np.isnan(r))
        yk, rk, stk = TM.step(rl, 0.0, INF, kind, nzn, g, keep_unconverged=True)
        assert stk["flags"] == 2 and stk["iterations"] == st["iterations"] and not np.all(np.isnan(yk))
    # g = 0: y = 0, no iteration
    y, r, st = TM.step(rl, 0.0, 1.0, 1, nz, np.zeros(N))
    assert st == {"flags": 0, "exit": 0, "iterations": 0, "resid": 0.0, "g_norm": 0.0, "step_norm": 0.0, "pred": 0.0}
    assert not y.any() and not r.any()


@pytest.mark.parametrize("N", [1, 2, 3])
def test_tiny_cases(N):
    colptr, rowval, nz, N = TM.tiny_case(N)
    rl = TM.RowLists(colptr, rowval, N)
    A = nz.reshape(N, N).T
    g = np.arange(1.0, N + 1)
    want = np.linalg.solve(A, -g)
    for kind in (0, 1):
        y, r, st = TM.step(rl, 0.0, INF, kind, nz, g)
        assert st["flags"] == 0 and st["exit"] == 0 and 1 <= st["iterations"] <= N
        assert np.linalg.norm(y - want) <= 16 * EPS * np.linalg.cond(A) * np.linalg.norm(want)
        delta = 0.25 * st["step_norm"]
        yb, rb, stb = TM.step(rl, 0.0, delta, kind, nz, g)
        assert stb["flags"] == 0 and stb["exit"] == 1 and abs(stb["step_norm"] - delta) <= BOUNDARY_C * EPS * delta
    y, r, st = TM.step(rl, 0.0, INF, 0, -nz, g)                  # negative definite
    assert st["flags"] == 2 and st["exit"] == 3 and st["iterations"] == 0
    y, r, st = TM.step(rl, 0.0, 2.0, 0, -nz, g)
    assert st["flags"] == 0 and st["exit"] == 2 and st["iterations"] == 1 and abs(st["step_norm"] - 2.0) <= BOUNDARY_C * EPS * 2.0


def test_abi_declares_and_exports_the_trust_region_consumer():
    names = ["csc_tr_create", "csc_tr_destroy", "csc_tr_set_options", "csc_tr_set_policy", "csc_tr_matvec_async", "csc_tr_step_async",
             "csc_tr_status"]
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    fd.lib.build()
    L = fd.lib.load()
    for n in names:
        assert re.search(r"^int fd_%s\(" % n, hdr, re.M), n
        assert hasattr(L, "fd_" + n) and "fd_" + n in fd.lib.EXPORTS
        assert "fd32_" + n not in hdr and "fd_" + n not in fd.lib.TYPED        # Float64 only, like the Hessian
    assert re.search(r"#define FD_CSC_TR_NORM_IDENTITY\s+0\b", hdr) and re.search(r"#define FD_CSC_TR_NORM_DIAG\s+1\b", hdr)
    assert "not checked" in hdr.lower() and "caller's contract" in hdr       # symmetry
    assert hasattr(fd, "CscTrustRegion")
    shim = open(os.path.join(ROOT, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    for n in names:
        assert ":fd_%s," % n in shim, n
    import torch
    if torch.cuda.is_available():
        return                                  # (the GPU tests create consumers)
    colptr, rowval = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int64)
    h = C.c_void_p()
    rc = L.fd_csc_tr_create(None, 2, colptr.ctypes.data, rowval.ctypes.data, 8, 0, 0, C.byref(h))
    assert rc == 7 and b"no HIP device" in L.fd_last_error()          # FD_ERR_NODEVICE
