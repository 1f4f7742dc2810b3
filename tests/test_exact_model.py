"""The exact host model (tests/exact_model.py) tied to the reference: it agrees with the C and numpy oracles on ordinary inputs at the
oracles' tolerance, its step sizes are within 4 ulps of an mpmath evaluation of max(relstep * sqrt(||x_c||_2), absstep) * dir at the
edges of the range (overflowing / underflowing sums of squares, subnormals, NaN / Inf coordinates), and the oracles take the same
edge semantics (NaN propagates through the step rule, the scaled norm where the plain sum leaves the range).  The general-pattern
pieces (sparse_f, rectangular colour_values, to_dense) against independent restatements, and the inputs of every case of
tests/test_gpu_exact_general.py evaluated with the model alone.  CPU only."""
import numpy as np
import pytest

import color_model
import exact_general as G
import exact_model as X
from finitediff_jl_amd import patterns as P
from oracle import np_oracle

mpmath = pytest.importorskip("mpmath")


def _mp_eps(x, colors0, c, fdtype, relstep, absstep, dir, dtype):
    """max(relstep * sqrt(||x_c||), absstep) [* dir] in 200-bit arithmetic, rounded to the element type -- the norm too, as the
    reference holds it (tmp = norm(x2) is an element-type value, src/jacobians.jl:560: a subnormal norm keeps a subnormal's bits)."""
    mp = mpmath.mp
    mp.prec = 200
    v = [mpmath.mpf(float(t)) for t in np.asarray(x)[np.asarray(colors0) == c]]
    if any(mpmath.isnan(t) for t in v):
        return np.dtype(dtype).type(np.nan)
    nrm = mpmath.mpf(float(np.dtype(dtype).type(float(mpmath.sqrt(mpmath.fsum([t * t for t in v]))))))
    a = mpmath.mpf(float(np.dtype(dtype).type(relstep))) * mpmath.sqrt(nrm)
    e = max(a, mpmath.mpf(float(np.dtype(dtype).type(absstep))))
    if fdtype == "forward":
        e = e * dir
    return np.dtype(dtype).type(float(e))


def _ulps(a, b, dtype):
    it = np.int64 if np.dtype(dtype) == np.float64 else np.int32
    ia, ib = np.asarray([a], dtype).view(it)[0], np.asarray([b], dtype).view(it)[0]
    return abs(int(ia) - int(ib))


def _edge_vector(case, N, C, rng, dtype):
    x = (rng.random(N) + 0.5).astype(dtype)
    c = np.arange(N) % C
    if case == "huge_1e240":
        x[c == 1] = 1e240 * (rng.random(int((c == 1).sum())) + 0.5)
    elif case == "huge_range":
        k = np.nonzero(c == 0)[0]
        x[k] = 10.0 ** rng.uniform(154, 300, k.size) * np.where(rng.random(k.size) < 0.5, -1, 1)
    elif case == "tiny_1e-200":
        x[c == 2] = 1e-200 * (rng.random(int((c == 2).sum())) + 0.5)
    elif case == "subnormal":
        x[c == 1] = 5e-324 * rng.integers(1, 1000, int((c == 1).sum()))
    elif case == "float32_huge":
        x[c == 0] = 1e36 * (rng.random(int((c == 0).sum())) + 0.1)      # (squares far past FLT_MAX, the norm inside the range)
    elif case == "float32_subnormal":
        x[c == 2] = 1.4e-45 * rng.integers(1, 1000, int((c == 2).sum()))
    return x.astype(dtype), c


EDGE = [("ordinary", np.float64, None), ("huge_1e240", np.float64, None), ("huge_range", np.float64, None),
        ("tiny_1e-200", np.float64, 0.0), ("subnormal", np.float64, 0.0), ("subnormal", np.float64, None),
        ("ordinary", np.float32, None), ("float32_huge", np.float32, None), ("float32_subnormal", np.float32, 0.0)]


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("case,dtype,absstep", EDGE)
@pytest.mark.parametrize("N,C", [(5, 3), (1000, 3), (70_001, 5)])
def test_model_eps_within_4_ulps_of_mpmath(fdtype, case, dtype, absstep, N, C):
    rng = np.random.default_rng(N + C)
    x, c = _edge_vector(case, N, C, rng, dtype)
    rel = X.default_relstep(fdtype, dtype)
    for dir in ((1.0, -1.0) if fdtype == "forward" else (1.0,)):
        eps, scaled = X.epsilons(x, c, C, fdtype, absstep=absstep, dir=dir, dtype=dtype)
        if case in ("huge_1e240", "huge_range", "tiny_1e-200") and dtype == np.float64 and N > 5:
            assert scaled.any(), case          # the case reaches the fallback
        for k in range(C):
            want = _mp_eps(x, c, k, fdtype, rel, rel if absstep is None else absstep, dir, dtype)
            assert np.isfinite(eps[k]), (case, k)
            assert _ulps(eps[k], want, dtype) <= 4, (case, k, eps[k], want)


def test_model_eps_nan_and_inf_coordinates():
    # one NaN, one +Inf and one -Inf coordinate, each in its own colour: NaN propagates (Julia's max), an infinite coordinate gives
    # an infinite step size; the other colours keep theirs
    N, C = 1000, 5
    x = np.random.default_rng(3).random(N) + 0.5
    c = np.arange(N) % C
    x[10] = np.nan        # colour 0
    x[21] = np.inf        # colour 1
    x[42] = -np.inf       # colour 2
    clean = x.copy()
    clean[[10, 21, 42]] = 1.0
    for fdtype in ("forward", "central"):
        eps, _ = X.epsilons(x, c, C, fdtype)
        ref, _ = X.epsilons(clean, c, C, fdtype)
        assert np.isnan(eps[0]) and eps[1] == np.inf and eps[2] == np.inf
        assert np.array_equal(eps[3:], ref[3:])
        for k in range(C):
            assert np.isnan(np_oracle.compute_epsilon(fdtype, np.sqrt(np_oracle.norm(np.where(c == k, x, 0.0), 1e-8, 1e-8)), 1e-8, 1e-8)) == (k == 0)


def test_model_plain_sum_is_the_defined_order():
    # at ordinary magnitudes the model's step sizes are those of eps_order (the device's defined summation order), bit for bit
    import eps_order
    rng = np.random.default_rng(1)
    for N, C in ((1, 1), (129, 3), (300_001, 9)):
        x = rng.random(N) - 0.5
        c = np.arange(N) % C
        for fdtype in ("forward", "central"):
            eps, scaled = X.epsilons(x, c, C, fdtype)
            assert not scaled.any()
            assert np.array_equal(eps, eps_order.epsilons(x, c, C, fdtype))


def _oracle_run(oracle, fam, prm, x, colors, fdtype, colptr, rowval, dtype=np.float64, **kw):
    return oracle.jacobian(fdtype, oracle.Fixture(fam, *prm, dtype=dtype), x, colors, kind=oracle.PAT_CSC_COMMON, colptr=colptr,
                           rowval=rowval, **kw)["out"]


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("fam,prm", [("tridiag", (1,)), ("tridiag_nl", (2,)), ("tridiag_nl", (1025,)), ("tridiag", (40_000,)),
                                     ("lap5", (6, 5)), ("lap5_nl", (64, 40)), ("lap5_nl", (254, 3))])
def test_model_agrees_with_the_c_oracle(oracle, fdtype, fam, prm):
    rng = np.random.default_rng(sum(prm))
    if fam.startswith("tridiag"):
        N = prm[0]
        colptr, rowval = P.tridiag_csc(N)
        colors = P.cyclic_colors(N, min(3, N) if N > 1 else 1)
    else:
        N = prm[0] * prm[1]
        colptr, rowval = P.lap5_csc(*prm)
        colors = P.lap5_colors(*prm)
    x = rng.random(N)
    c0 = colors - 1
    C = int(colors.max())
    for dir in ((1.0, -1.0) if fdtype == "forward" else (1.0,)):
        eps, _ = X.epsilons(x, c0, C, fdtype, dir=dir)
        D = X.colour_values(X.fixture(fam, *prm), x, c0, C, eps, fdtype)
        got = X.to_csc(D, c0, colptr, rowval)
        ref = _oracle_run(oracle, fam, prm, x, colors, fdtype, colptr, rowval, dir=dir)
        # the oracle's later colours see x drifted by the in-place un-perturbation: the existing tolerance (test_gpu_parity._tol_ok)
        atol = 16 * np.finfo(np.float64).eps * 8.0 / np.min(np.abs(eps))
        assert np.all(np.abs(got - ref) <= 1e-6 * np.abs(ref) + atol), (fam, prm, fdtype, np.max(np.abs(got - ref)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_model_agrees_with_the_float32_and_float64_oracles_on_storage_layouts(oracle, dtype):
    # the Banded and Tridiagonal layouts hold the CSC values at their slots
    N = 1000
    x = np.random.default_rng(4).random(N).astype(dtype)
    colors = P.cyclic_colors(N, 3)
    c0 = colors - 1
    colptr, rowval = P.tridiag_csc(N)
    eps, _ = X.epsilons(x, c0, 3, "central", dtype=dtype)
    D = X.colour_values(X.fixture("tridiag_nl", N), x, c0, 3, eps, "central")
    csc = X.to_csc(D, c0, colptr, rowval)
    dense = P.csc_to_dense(N, N, colptr, rowval, csc)
    band = X.to_banded(D, c0, N, N, 1, 1).reshape(N, 3)
    dl, d, du = X.to_tridiagonal(D, c0, N)
    assert np.array_equal(band[:, 1], np.diag(dense)) and np.array_equal(band[1:, 0], np.diag(dense, 1))
    assert np.array_equal(band[:-1, 2], np.diag(dense, -1)) and band[0, 0] == 0 and band[-1, 2] == 0
    assert np.array_equal(dl, np.diag(dense, -1)) and np.array_equal(d, np.diag(dense)) and np.array_equal(du, np.diag(dense, 1))
    ref = _oracle_run(oracle, "tridiag_nl", (N,), x, colors, "central", colptr, rowval, dtype=dtype)
    tol = (1e-6, 1e-6) if dtype == np.float64 else (1e-3, 1e-2)
    assert np.all(np.abs(csc.astype(np.float64) - ref) <= tol[0] * np.abs(ref) + tol[1])


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("case,absstep", [("huge_1e240", None), ("huge_range", None), ("tiny_1e-200", 0.0)])
def test_oracles_take_the_scaled_norm(oracle, fdtype, case, absstep):
    # before the fallback, the oracles' plain sum of squares overflowed (eps = Inf: every value of the colour NaN) or flushed the
    # squares (eps = absstep); now both give the model's values within their tolerance.  tridiag (linear): J = -2 / 1 wherever
    # x + eps does not absorb eps
    N, C = 3000, 3
    x, c0 = _edge_vector(case, N, C, np.random.default_rng(9), np.float64)
    colors = c0 + 1
    colptr, rowval = P.tridiag_csc(N)
    eps, scaled = X.epsilons(x, c0, C, fdtype, absstep=absstep)
    assert scaled.any()
    D = X.colour_values(X.fixture("tridiag_nl", N), x, c0, C, eps, fdtype)
    want = X.to_csc(D, c0, colptr, rowval)
    ref = _oracle_run(oracle, "tridiag_nl", (N,), x, colors, fdtype, colptr, rowval, absstep=absstep)
    assert np.all(np.isfinite(ref)) == np.all(np.isfinite(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(ref[fin] - want[fin]) <= 1e-6 * np.abs(want[fin]) + 1e-6 * np.max(np.abs(want[fin])))
    A = P.csc_to_dense(N, N, colptr, rowval, np.ones(rowval.size)).astype(bool)
    rel = X.default_relstep(fdtype)
    Jn, _ = np_oracle.jacobian(lambda fx, xx: fx.__setitem__(slice(None), X.tridiag_f(xx, True)), x, colors, A, fdtype,
                               relstep=rel, absstep=rel if absstep is None else absstep)
    got_n = Jn[rowval - 1, np.repeat(np.arange(N), np.diff(colptr))]
    assert np.all(np.isfinite(got_n) == np.isfinite(want))
    assert np.all(np.abs(got_n[fin] - want[fin]) <= 1e-6 * np.abs(want[fin]) + 1e-6 * np.max(np.abs(want[fin])))


@pytest.mark.parametrize("fdtype", ["forward", "central"])
def test_float32_oracles_take_the_scaled_norm_without_overflow(oracle, fdtype):
    # Float32 elements: the oracles' fallback sums in double WITHOUT scaling (a float's square cannot leave double's range; 2^600
    # would overflow it).  One colour holds a single tiny coordinate, the rest are 0, absstep = 0: the step sizes stay finite and no
    # value turns NaN (a step of Inf would poison every later colour through x1 - Inf * mask).
    N = 30
    colors = P.cyclic_colors(N, 3)
    x = (np.random.default_rng(2).random(N) + 0.5).astype(np.float32)
    x[colors == 2] = 0.0
    x[4] = np.float32(2.0 ** -61)             # colour 2 (0-based 1): its only non-zero coordinate
    colptr, rowval = P.tridiag_csc(N)
    ref = _oracle_run(oracle, "tridiag_nl", (N,), x, colors, fdtype, colptr, rowval, dtype=np.float32, absstep=0.0)
    assert not np.isnan(ref).any()
    eps, scaled = X.epsilons(x, colors - 1, 3, fdtype, absstep=0.0, dtype=np.float32)
    assert np.isfinite(eps).all() and (eps > 0).all()
    for v, absstep in ((1e30, None), (1e-30, 0.0), (3e38, None), (1.4e-45, 0.0)):
        y = np.zeros(8, np.float32)
        y[0] = v
        rel = 1e-4
        got = np_oracle.norm(y, rel, rel if absstep is None else absstep)
        assert got == np.float64(np.float32(v)), (v, got)


def test_oracles_nan_coordinate_poisons_only_its_colour(oracle):
    # Julia's Bool is a strong zero (x * false == 0 even for NaN): a NaN in the LAST colour gives that colour a NaN step and NaN
    # columns, and leaves the earlier colours' values finite in both oracles (no later colour for the in-place un-perturbation to reach)
    N, C = 300, 3
    x = np.random.default_rng(5).random(N) + 0.5
    x[2] = np.nan                              # colour 3
    colors = P.cyclic_colors(N, C)
    colptr, rowval = P.tridiag_csc(N)
    cols = np.repeat(np.arange(N), np.diff(colptr))
    A = P.csc_to_dense(N, N, colptr, rowval, np.ones(rowval.size)).astype(bool)
    rows_nan = np.zeros(N, bool)
    rows_nan[1:4] = True                       # the rows x[2] enters
    for fdtype in ("forward", "central"):
        ref = _oracle_run(oracle, "tridiag_nl", (N,), x, colors, fdtype, colptr, rowval)
        Jn, _ = np_oracle.jacobian(lambda fx, xx: fx.__setitem__(slice(None), X.tridiag_f(xx, True)), x, colors, A, fdtype)
        got_n = Jn[rowval - 1, cols]
        for out in (ref, got_n):
            last = colors[cols] == C
            assert np.isnan(out[last]).all()
            # earlier colours: NaN only in the rows x[2] itself enters (f(x) there is NaN), finite everywhere else
            other = ~last & ~(rows_nan[rowval - 1] & (fdtype == "forward"))
            other &= ~rows_nan[rowval - 1]
            assert np.isfinite(out[other]).all()


# ---- the general-pattern anchor: sparse_f, rectangular residuals, the dense-J destination, the cases of test_gpu_exact_general.py ----
@pytest.mark.parametrize("pname", ["random_band600", "tall", "wide", "ragged"])
def test_sparse_f_equals_the_float64_restatement_bit_for_bit(pname):
    # tests/test_gpu_storetable.py::sparse_np_factory is the Float64 restatement the oracle comparisons use: a random band, M > N,
    # M < N (rows of up to 61 entries), and the ragged pattern (empty rows and columns, one row of 3000 entries: the cumsum branch)
    from test_gpu_storetable import sparse_np_factory
    M, N, colptr, rowval = G.pattern(pname)
    cnt = np.bincount(rowval - 1, minlength=M)
    if pname == "ragged":
        assert (cnt == 0).any() and (np.diff(colptr) == 0).any() and cnt.max() == 3000
    if pname == "wide":
        assert cnt.max() > 32
    rng = np.random.default_rng(M + N)
    x = rng.random(N) - 0.25
    x[rng.random(N) < 0.05] = -0.0
    want = np.full(M, np.nan)
    sparse_np_factory(M, N, colptr, rowval)(want, x)
    got = X.fixture("sparse", M, N, colptr, rowval)(x)
    assert got.dtype == np.float64 and X.same_bits(got, want).all()
    assert not np.signbit(got[cnt == 0]).any()                   # an empty row is +0
    # the element type is the argument's: Float32 in, Float32 arithmetic (the Float64 sum of the same terms differs)
    g32 = X.fixture("sparse", M, N, colptr, rowval)(x.astype(np.float32))
    assert g32.dtype == np.float32 and np.allclose(g32, want, rtol=1e-4 * max(1, cnt.max()) ** 0.5, atol=1e-5)


@pytest.mark.parametrize("pname", ["random_band600", "tall", "wide"])
def test_model_forward_jacobian_against_the_analytic_one(pname):
    """f_r = sum_j w(r, j) phi(x_j), phi(v) = v + v^2 / 4: dJ[r, j] = w (1 + x_j / 2).  With a VALID colouring exactly one term of row r
    moves, t(v) = w (v + v^2 / 4), and in exact arithmetic (t(v + e) - t(v)) / e = w (1 + v / 2) + w e / 4: the truncation term of this
    quadratic is exactly w eps_c / 4.

    ASSERTED: |error| <= w eps_c / 4 + 4 len_r u max|term| / eps_c with u = 2^-52 and max|term| the largest term of row r -- the bound
    the general-pattern anchor is specified with.  Its rounding part counts, per evaluation, the moved term's 3 roundings ((q v) v,
    v + ., w .; q v is exact) and the row's len_r - 1 additions at (u / 2) of ONE term's size each, plus the point's own rounding
    (fl(v + e) differs from v + e by at most (u / 2) (v + e), which moves the numerator by t'(v) (u / 2) (v + e) <= 1.2 (u / 2) t):
    (2 len_r + 5.2) (u / 2) max|term| <= 4 len_r u max|term| for every len_r >= 1.  An addition's error scales with its partial sum, not
    with one term, so for a long row this count is a first-order one (errors of independent sign; on these patterns the worst ratio
    is 0.49 / 0.76 / 0.19 of the bound), not a worst case.

    ALSO ASSERTED, weaker: the same expression with S_r, the row's value, in place of max|term|.  With x > 0 all terms are positive, S_r
    bounds every partial sum and every term, and the count above is then a rigorous worst case."""
    M, N, colptr, rowval = G.pattern(pname)
    colors = G.colouring(pname, "greedy")
    assert color_model.valid(M, colptr, rowval, colors)
    c0, C = colors - 1, int(colors.max())
    x = np.random.default_rng(N).random(N) + 0.1
    f = X.fixture("sparse", M, N, colptr, rowval)
    u = 2.0 ** -52
    cols, rows = P.csc_cols(colptr) - 1, rowval - 1
    w = 1.0 + 0.125 * ((rows + 3 * cols) & 7)
    n = np.bincount(rows, minlength=M)[rows]
    for dir in (1.0, -1.0):
        eps, scaled = X.epsilons(x, c0, C, "forward", dir=dir)
        assert not scaled.any()
        got = X.to_csc(X.colour_values(f, x, c0, C, eps, "forward"), c0, colptr, rowval)
        e = np.abs(eps[c0[cols]])
        xs = x + np.abs(eps).max()                                # (every coordinate at its largest: terms grow with v > 0)
        term = w * (xs[cols] + (0.25 * xs[cols]) * xs[cols])
        tmax = np.zeros(M)
        np.maximum.at(tmax, rows, term)
        err = np.abs(got - w * (1.0 + 0.5 * x[cols]))
        bound = w * e / 4 + 4 * n * u * tmax[rows] / e
        assert (err <= bound).all(), (pname, float(np.max(err / bound)))
        assert (err > 0.1 * bound).any()                          # (the bound is of the error's own size, not a blanket)
        assert (err <= w * e / 4 + 4 * n * u * f(xs)[rows] / e).all()


def test_model_layouts_against_an_entry_by_entry_assembly():
    # 7 x 5, one column without a colour, one empty column, one empty row: to_csc and to_dense against a plain Python loop
    M, N = 7, 5
    A = np.zeros((M, N), bool)
    for r, j in [(0, 0), (2, 0), (6, 0), (1, 1), (2, 1), (3, 2), (6, 2), (0, 4), (4, 4), (6, 4)]:      # (column 3 and row 5 are empty)
        A[r, j] = True
    colptr, rowval = P.csc_from_dense(A)
    colors = np.array([1, 2, 0, 3, 2])                            # column 2 has no colour
    c0, C = colors - 1, 3
    D = np.random.default_rng(0).random((C, M)) + 1.0
    csc = X.to_csc(D, c0, colptr, rowval)
    dense = X.to_dense(D, c0, colptr, rowval, M, N)
    want_dense = np.zeros((M, N))
    want_csc = []
    for j in range(N):
        for r in range(M):
            if A[r, j]:
                v = D[colors[j] - 1, r] if colors[j] > 0 else 0.0
                want_dense[r, j] = v
                want_csc.append(v)
    assert dense.shape == (M, N) and dense.flags.f_contiguous
    assert np.array_equal(csc, np.array(want_csc)) and np.array_equal(dense, want_dense)
    assert np.all(csc[colptr[2] - 1:colptr[3] - 1] == 0) and np.all(dense[~A] == 0)
    # rectangular residuals: D is (C, M), and a caller's f_in is what a forward difference subtracts
    f = X.fixture("sparse", M, N, colptr, rowval)
    x = np.random.default_rng(1).random(N)
    eps, _ = X.epsilons(x, c0, C, "forward")
    fin = np.arange(M, dtype=np.float64)
    for fdtype in ("forward", "central"):
        assert X.colour_values(f, x, c0, C, eps, fdtype).shape == (C, M)
    shifted = X.colour_values(f, x, c0, C, eps, "forward", f_in=fin)
    xp = np.where(c0 == 1, x + eps[1], x + 0.0)
    assert X.same_bits(shifted[1], (f(xp) - fin) / eps[1]).all()


def test_general_colourings_are_what_their_names_say():
    for pname in ("random_band", "random_band600", "ragged", "wide", "tall", "lap5", "tiny_65", "tiny_257"):
        M, N, colptr, rowval = G.pattern(pname)
        g, n5, inv = (G.colouring(pname, k) for k in ("greedy", "none5", "invalid"))
        assert color_model.valid(M, colptr, rowval, g) and g.min() >= 1
        assert color_model.valid(M, colptr, rowval, n5) and (n5 == 0).sum() == 5
        assert not color_model.valid(M, colptr, rowval, inv) and inv.max() <= 6 and inv.min() >= 1
        for c in (g, inv):                                        # not cyclic: the step-size reduction reads the colours
            assert not np.array_equal(c, (np.arange(N) + c[0] - 1) % c.max() + 1)
    M, N, colptr, rowval = G.pattern("lap5")
    for kind in ("stencil", "stencil_none5"):
        c = G.colouring("lap5", kind)
        assert color_model.valid(M, colptr, rowval, c) and c.max() == 5 and (c == 0).sum() == (5 if kind == "stencil_none5" else 0)
        assert not np.array_equal(c, (np.arange(N) + c[0] - 1) % 5 + 1)
    assert G.colouring("random_band", "greedy").max() > 8         # per-colour lists, k_eps_finalize
    assert G.colouring("ragged", "greedy").max() >= 3000          # (one colour per column of the dense row: Int32 colours)


_KEYS = {}
for _c in G.CASES:
    _KEYS.setdefault(G.model_key(_c), _c)


@pytest.mark.parametrize("case", list(_KEYS.values()), ids=[c["id"] for c in _KEYS.values()])
def test_general_cases_keep_most_stored_values_finite(case):
    # the condition under which a bit-for-bit comparison of a case means something: at least 90 % of the stored values are finite
    # (a NaN matches any NaN).  few_huge must reach the scaled norm, nan_inf a non-finite step size.
    want, eps, scaled = G.model(case)
    assert want.size > 0
    frac = float(np.isfinite(want).mean())
    assert frac >= G.MIN_FINITE, (case["id"], frac)
    if case["family"] == "few_huge":
        assert scaled.any() and np.isfinite(eps).all() and frac < 1.0
    if case["family"] == "nan_inf":
        assert np.isnan(eps).any() and frac < 1.0
    if case["family"] == "cancel":              # the 1e30 columns are one colour's, and every x + eps is absorbed: zero numerators
        inp = G.inputs(case)
        assert np.unique(inp["colors"][inp["x"] >= 1e30]).size == 1 and (inp["x"] >= 1e30).sum() > 8
        assert np.isfinite(eps).all() and (want == 0).all()
    if case["family"] in ("tiny_1e-200", "subnormal") and case["dtype"] == "f64":
        assert scaled.any()


# ---- the cases of tests/test_gpu_exact_store.py (the storing routes of general patterns), evaluated with the model alone ----------------
import exact_store_cases as S

_SKEYS = {}
for _c in S.CASES:
    _SKEYS.setdefault(S.model_key(_c), _c)


def test_lap7_fixture_against_a_point_by_point_restatement():
    # FD_F_LAP7 (lap7_row, csrc/fdjac_functor_f.hip) one grid point at a time in Python floats -- IEEE doubles, the kernel's order:
    # ((((((d + s) + w) + e) + n) + u) - 6 c) + (c c) e, a neighbour outside the grid is 0 -- on the three grids of the store cases
    for name, (nx, ny, nz) in S.LAP7.items():
        N = nx * ny * nz
        rng = np.random.default_rng(N)
        x = rng.random(N) - 0.25
        x[rng.random(N) < 0.1] = -0.0
        got = X.fixture("lap7", nx, ny, nz)(x)
        want = np.empty(N)
        at = lambda i, j, l: float(x[i + nx * (j + ny * l)]) if (0 <= i < nx and 0 <= j < ny and 0 <= l < nz) else 0.0
        for k in range(N):
            i, j, l = k % nx, (k // nx) % ny, k // (nx * ny)
            c, e = at(i, j, l), at(i + 1, j, l)
            want[k] = ((((((at(i, j, l - 1) + at(i, j - 1, l)) + at(i - 1, j, l)) + e) + at(i, j + 1, l)) + at(i, j, l + 1)) - 6.0 * c) + (c * c) * e
        assert got.dtype == np.float64 and X.same_bits(got, want).all(), name
        g32 = X.fixture("lap7", nx, ny, nz)(x.astype(np.float32))
        assert g32.dtype == np.float32 and np.allclose(g32, want, rtol=1e-4, atol=1e-5)
        # the pattern of the cases is the row's own support, the grid's seven colours are valid for it
        M, N2, colptr, rowval = S.pattern(name)
        assert (M, N2) == (N, N) and color_model.valid(M, colptr, rowval, S.colouring(name, "greedy"))


def test_store_patterns_and_colourings_are_what_their_names_say():
    M, N, colptr, rowval = S.pattern("ragged400")
    cnt = np.bincount(rowval - 1, minlength=M)
    assert (cnt == 0).any() and (np.diff(colptr) == 0).any() and (cnt == 1).any() and cnt.max() == 40 > 32
    M, N, colptr, rowval = S.pattern("rows12")
    tiles = np.add.reduceat(np.bincount(rowval - 1, minlength=M), np.arange(0, M, 256))
    assert M == N == 3000 and tiles[:-1].min() > 3072, tiles           # (every full tile overflows the staged run)
    for pname in ("random_band", "ragged400", "rows12", "lap7_33x4x9"):
        M, N, colptr, rowval = S.pattern(pname)
        for kind in ("greedy", "many", "none5") + (("small",) if pname in S.LAP7 else ("invalid6",)):
            c = S.colouring(pname, kind)
            assert color_model.valid(M, colptr, rowval, c) == (kind != "invalid6"), (pname, kind)
        assert S.colouring(pname, "many").max() > 8 and (S.colouring(pname, "none5") == 0).sum() == 5
        assert not color_model.valid(M, colptr, rowval, S.colouring(pname, "ones"))
    fams = {(c["route"], c["fdtype"], c["dir"]) for c in S.CASES if c["family"] == "signed_zeros"}
    for route in ("cols", "win", "rows", "ents", "lap7", "jit", "terms", "terms_ents"):
        assert (route, "forward", -1.0) in fams, route                # signed zeros meet dir = -1 on every route
        have = {c["family"] for c in S.CASES if c["route"] == route and c["dtype"] == "f64"}
        assert have >= set(S.FAMILIES64), (route, set(S.FAMILIES64) - have)


@pytest.mark.parametrize("case", list(_SKEYS.values()), ids=[c["id"] for c in _SKEYS.values()])
def test_store_cases_keep_most_stored_values_finite_and_reach_their_edge(case):
    """The finite share (exact_general.MIN_FINITE) and, for the families named after an edge of the division, that the case reaches it:
    the quotients sorted by the fall-back rules of fd_div_shared on the model's own numerators and divisors (S.div_sides).

    rule3 is the three-argument form every store route calls: it looks at |a y| and |a| only.  rule4, the four-argument form (no route
    calls it; restated because the operand families were cut for it), also tests the divisor.  What each family must populate:
      eps_2p100_in    forward: the divisor is 2^100 itself -- product under both rules.  central: the divisor is 2^101 -- rule4 divides
      eps_2p100_out   the divisor lies just outside 2^100: rule3 still takes the product (forward), rule4 divides -- the two rules part here
      eps_2m100_*     x + eps is absorbed: every numerator is 0 -- both rules divide (0 lies below 2^-900)
      num_2p800       numerators from below 2^800 to above 2^900: rule3 populated on BOTH sides; the step 1e136 is outside rule4's range
      num_2m900       every numerator non-zero and below 2^-900, the quotients of order 1: rule3 divides (its lower edge, with a
                      numerator at which a wrong condition would show -- the zero numerators of eps_2m100_* divide to 0 either way)
      tiny / subnorm. step sizes near 1e-108 / 1e-168: product under rule3, division under rule4 (|b| < 2^-100)
    Across these families both sides of both rules are populated (asserted by test_store_cases_populate_both_sides_of_the_division)."""
    want, eps, scaled = S.model(case)
    assert want.size > 0
    frac = float(np.isfinite(want).mean())
    assert frac >= S.MIN_FINITE, (case["id"], frac)
    fam, fwd = case["family"], case["fdtype"] == "forward"
    if fam == "nan_inf":
        assert np.isnan(eps).any() and frac < 1.0
    if fam == "cancel":
        assert np.isfinite(eps).all() and (want == 0).all()
    if fam in ("tiny_1e-200", "subnormal") and case["dtype"] == "f64":
        assert scaled.any()
    if fam in S.DIV_FAMILIES:
        assert case["dtype"] == "f64"
        d = S.div_sides(case)
        (p3, d3), (p4, d4) = d["rule3"], d["rule4"]
        assert p3 + d3 == p4 + d4 > 0
        if fam == "eps_2p100_in":
            assert d["b"] == ((2.0 ** 100,) * 2 if fwd else (2.0 ** 101,) * 2)
            assert (p3 > 0 and p4 == p3 and d4 == d3) if fwd else (p4 == 0 and d4 > 0), d
        elif fam == "eps_2p100_out":
            assert 2.0 ** 100 < d["b"][0] < 2.0 ** 100 * (1 + 2.0 ** -39) or not fwd
            assert p4 == 0 and d4 > 0 and (p3 > 0 or not fwd), d
        elif fam in ("eps_2m100_in", "eps_2m100_out"):
            assert p3 == 0 and d3 > 0 and p4 == 0 and (want == 0).all(), d
        elif fam == "num_2p800":
            assert p3 > 0 and d3 > 0 and p4 == 0 and frac == 1.0, d
        elif fam == "num_2m900":
            assert p3 == 0 and d3 > 0 and p4 == 0 and frac == 1.0 and (want != 0).all() and (np.abs(want) > 0.4).all() and (np.abs(want) < 40).all(), d
        else:
            assert p3 > 0 and d3 == 0 and p4 == 0 and d["b"][1] < 2.0 ** -100, d


def test_store_cases_populate_both_sides_of_the_division():
    tot = {"rule3": [0, 0], "rule4": [0, 0]}
    for case in _SKEYS.values():
        if case["family"] in S.DIV_FAMILIES and case["route"] in ("cols", "lap7"):
            d = S.div_sides(case)
            for k in tot:
                tot[k][0] += d[k][0]
                tot[k][1] += d[k][1]
    assert all(min(v) > 0 for v in tot.values()), tot
