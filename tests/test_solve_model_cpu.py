"""tests/solve_model.py checked on the CPU: the references against mpmath, family E against SciPy and the host models, and the two
facts that justify tests/test_gpu_solve_longrange.py -- its inputs DISCRIMINATE (a wrong coupling at any level of the elimination, or
in any rank's spike tips, fails the very assertion the GPU test makes) and the older solver tests' inputs do NOT (the same faults from
the second level up stay inside their 1e-11)."""
import numpy as np
import pytest
import scipy.linalg

import solve_model as M
import solver_inputs as SI

MODES = ("zero", "flip")


# ------------------------------------------------------------------------------------------------------------ references
def _mp_banded_solve(mpmath, A, N, b):
    """Pivot-free banded elimination at 50 digits (the matrices are diagonally dominant or SPD)."""
    mp = mpmath.mp
    mp.dps = 50
    lo, up = -min(A), max(A)
    rows = [{i + k: mpmath.mpf(float(v[i])) for k, v in A.items() if 0 <= i + k < N and (v[i] != 0 or k == 0)} for i in range(N)]
    d = [mpmath.mpf(float(x)) for x in b]
    for i in range(N):
        piv = rows[i][i]
        for r in range(i + 1, min(N, i + lo + 1)):
            f = rows[r].pop(i, None)
            if f is None or f == 0:
                continue
            f = f / piv
            for j, v in rows[i].items():
                if j > i:
                    rows[r][j] = rows[r].get(j, 0) - f * v
            d[r] -= f * d[i]
    x = [mpmath.mpf(0)] * N
    for i in range(N - 1, -1, -1):
        x[i] = (d[i] - sum(v * x[j] for j, v in rows[i].items() if j > i)) / rows[i][i]
    return x


S_SMALL = [lambda: M.s_tridiag(2000, 64.0, 1), lambda: M.s_tridiag(1500, 512.0, 2, np.float32), lambda: M.s_tridiag(700, 4096.0, 3, shift=(0.0, -2.0)),
           lambda: M.s_banded(1200, 2, 2, 300.0, 4), lambda: M.s_banded(900, 1, 2, 200.0, 5), lambda: M.s_banded(800, 4, 0, 200.0, 6),
           lambda: M.s_banded(1000, 0, 2, 250.0, 7, np.float32), lambda: M.s_banded(600, 4, 4, 150.0, 8),
           lambda: M.s_block_dominant(60, 5, 15.0, 9), lambda: M.s_block_dominant(20, 16, 5.0, 10, np.float32),
           lambda: M.s_block_dense(50, 4, 12.0, 11), lambda: M.s_block_dense(12, 16, 3.0, 12, np.float32)]


@pytest.mark.parametrize("make", S_SMALL, ids=[str(k) for k in range(len(S_SMALL))])
def test_refined_reference_equals_a_50_digit_solve(make):
    mpmath = pytest.importorskip("mpmath")
    s = make()
    x, E = M.refined_reference(s)
    want = _mp_banded_solve(mpmath, s.A, s.N, s.b)
    nrm = max(abs(v) for v in want)
    err = max(abs(mpmath.mpf(float(np.float64(x[i]))) + mpmath.mpf(float(x[i] - np.float64(x[i]))) - want[i]) for i in range(s.N))
    assert err <= 4 * np.finfo(np.float64).eps * nrm, (float(err / nrm), E)          # 4 ulp of Float64 at the solution's norm


def test_spd_block_condition():
    for bs in (4, 5, 16, 31, 32):
        G = M.spd_block(bs, np.random.default_rng(bs))
        assert np.linalg.cond(G) <= 4.0 and np.all(np.linalg.eigvalsh(G) > 0)
        assert np.any(np.abs(G).sum(1) - 2 * np.diag(G) > 0) or bs <= 5           # (rows of T (x) G are never dominant: 2 G_ii off the block)


# ------------------------------------------------------------------------------------------------------------ family E self-checks
def _dense(s):
    return M.to_sparse(s.A, s.N).toarray()


@pytest.mark.parametrize("shift", M.E_SHIFTS)
def test_family_e_closed_form_is_the_solution_and_the_models_reproduce_it(shift):
    cases = [M.e_tridiag(N, 3, kind, shift) for kind in ("lower", "upper", "segmented") for N in (1, 2, 9, 513, 2113, 4097)]
    cases += [M.e_tridiag(70001, 4, "segmented", shift), M.e_tridiag(40000, 5, "lower", shift, np.float32)]
    for s in cases:
        assert s.y.dtype == np.int64
        assert np.array_equal(M.TriModel(*M.tri_rows(s)).solve(), s.y.astype(np.float64)), ("tri", s.N)
        if s.N <= 5000:
            assert np.array_equal(scipy.linalg.solve(_dense(s), s.b.astype(np.float64)), s.y)
            D, lo, up = s.A[0], s.A[-1], s.A[1]
            p = np.arange(s.N) - (lo != 0) + (up != 0)
            assert np.array_equal(M.forest_solution(D, lo + up, p, s.b), s.y)       # the O(N) prefix sums against pointer doubling
    for (N, l, u) in [(7, 2, 2), (1000, 2, 2), (4097, 2, 1), (2049, 0, 2), (3000, 4, 0), (2047, 3, 3), (4000, 4, 4)]:
        for lower in (True, False):
            if (l if lower else u) == 0:
                continue
            s = M.e_banded(N, l, u, 6, lower, shift)
            assert all(-l <= k <= u for k in s.A)
            assert np.array_equal(scipy.linalg.solve(_dense(s), s.b), s.y)
            assert np.array_equal(M.BcrModel(*M.bcr_blocks(s, M.band_K(l, u))).solve().reshape(-1)[:N], s.y.astype(np.float64))
    for nb, bs in [(1, 32), (2, 32), (3, 31), (7, 5), (100, 16), (1025, 4), (50, 1)]:
        for lower in (True, False):
            s = M.e_block(nb, bs, 7, lower, shift)
            seen = M.block_seen(s.J, nb, bs, s.alpha, s.beta)
            assert set(seen) == set(s.A) and all(np.array_equal(seen[k], s.A[k]) for k in seen)
            if s.N <= 5000:
                assert np.array_equal(scipy.linalg.solve(_dense(s), s.b), s.y)
            assert np.array_equal(M.BcrModel(*M.bcr_blocks(s, bs)).solve().reshape(-1), s.y.astype(np.float64))


def test_family_e_is_weakly_dominant_with_a_chain_across_every_cut():
    for N, cuts in M.TRI_SHARDED:
        s = M.e_tridiag_crossing(N, cuts, 47 + N)
        assert np.all(np.abs(s.A[0]) == 1) and np.all(np.abs(s.A[-1]) + np.abs(s.A[1]) <= 1)
        assert np.array_equal(M.tri_sharded_model(*M.tri_rows(s), cuts), s.y.astype(np.float64))
        assert M.sharded_lam(cuts) >= 2 * max(np.diff(cuts))


# ------------------------------------------------------------------------------------------------------------ discrimination
def _fails(kind, x, want, tol):
    """Does x fail the GPU test's assertion?  E: any element differs; S: the error is >= 100 x the tolerance."""
    return bool(np.any(x != want)) if kind == "E" else float(np.max(np.abs(x - want))) >= 100.0 * tol


def _discriminates(model, kind, y, tol, pad_to=None):
    for L in model.fault_levels:
        idx = model.level_rows(L)
        for mode in MODES:
            x = model.with_fault(L, mode).solve(down_to=L)           # the unknowns of level L are elements of y
            if pad_to is None:
                ok = idx >= 0
                got, want = x[ok], y[idx[ok]]
            else:
                got, want = x, pad_to[idx]
            assert _fails(kind, got, want, tol), (kind, L, mode, len(model.ns))


def _s_ref(s, dtype=np.float64):
    x, E = M.refined_reference(s)
    y = np.asarray(x, np.float64)
    return y, M.s_tolerance(y, E, dtype)


@pytest.mark.parametrize("N", [N for N in M.TRI_E_N if len(M.tri_levels(N)) > 1])
def test_tridiagonal_cases_discriminate_at_every_level(N):
    k = M.TRI_E_N.index(N)
    sysE = M.e_tridiag(N, 11 + N, "segmented", M.E_SHIFTS[k % 4])
    _discriminates(M.TriModel(*M.tri_rows(sysE)), "E", sysE.y.astype(np.float64), 0.0)
    lams = [lam for n, lam in M.TRI_S_CASES if n == N]
    for q, lam in enumerate(lams):
        sysS = M.s_tridiag(N, lam, (13 + N) if q == 0 else 29)
        y, tol = _s_ref(sysS)
        _discriminates(M.TriModel(*M.tri_rows(sysS)), "S", y, tol)


def test_tridiagonal_special_cases_discriminate():
    for N in M.TRI_SCHEDULE_N:
        sysE = M.e_tridiag(N, 31 + N, "segmented", M.E_SHIFTS[N % 4])
        _discriminates(M.TriModel(*M.tri_rows(sysE)), "E", sysE.y.astype(np.float64), 0.0)
        sysS = M.s_tridiag(N, M.tri_default_lam(N), 37 + N)
        y, tol = _s_ref(sysS)
        _discriminates(M.TriModel(*M.tri_rows(sysS)), "S", y, tol)
    for kind in ("lower", "upper"):
        for N in [N for N in M.TRI_CHAIN_N if len(M.tri_levels(N)) > 1]:
            for q, shift in enumerate(M.E_SHIFTS):
                s = M.e_tridiag(N, 17 + q, kind, shift)
                _discriminates(M.TriModel(*M.tri_rows(s)), "E", s.y.astype(np.float64), 0.0)
    s = M.e_tridiag(3 * 10 ** 6 + 1, 23, "segmented", (2.0, -1.0))           # the other family of test_tridiagonal_slowest_decay
    _discriminates(M.TriModel(*M.tri_rows(s)), "E", s.y.astype(np.float64), 0.0)
    f32 = np.float32
    s = M.e_tridiag(M.TRI_F32, 41, "segmented", (2.0, -1.0), dtype=f32)
    _discriminates(M.TriModel(*M.tri_rows(s)), "E", s.y.astype(np.float64), 0.0)
    s = M.s_tridiag(M.TRI_F32, M.tri_default_lam(M.TRI_F32), 43, dtype=f32)
    y, tol = _s_ref(s, f32)
    _discriminates(M.TriModel(*M.tri_rows(s)), "S", y, tol)


@pytest.mark.parametrize("N,cuts", M.TRI_SHARDED)
def test_sharded_cases_discriminate_in_every_ranks_tips(N, cuts):
    sysE = M.e_tridiag_crossing(N, cuts, 47 + N)
    sysS = M.s_tridiag(N, M.sharded_lam(cuts), 53 + N)
    yS, tol = _s_ref(sysS)
    # family S is two-sided: every rank's tips matter.  A family-E chain crosses a cut in ONE direction (a forest has no 2-cycle): the
    # tips of a rank are used only where a chain runs through it (solve_model.through_ranks) -- there the faulted model must fail
    W = len(cuts) - 1
    through = M.through_ranks(sysE, cuts)
    assert all(r in through for r in range(1, W - 1) if cuts[r + 1] - cuts[r] <= 8)
    for r in range(W):
        for mode in MODES:
            if r in through:
                assert _fails("E", M.tri_sharded_model(*M.tri_rows(sysE), cuts, tip_fault=(r, mode)), sysE.y, 0.0), (r, mode)
            assert _fails("S", M.tri_sharded_model(*M.tri_rows(sysS), cuts, tip_fault=(r, mode)), yS, tol), (r, mode)


@pytest.mark.parametrize("N,l,u", M.BAND_SHAPES)
def test_banded_cases_discriminate_at_every_level(N, l, u):
    q = M.BAND_SHAPES.index((N, l, u))
    K = M.band_K(l, u)

    def padded(y, n):
        out = np.zeros(n * K); out[:N] = y
        return out.reshape(n, K)

    for dtype in (np.float64, np.float32):
        sysS, _ = M.gpu_band_systems(N, l, u, dtype)
        y, tol = _s_ref(sysS, dtype)
        model = M.BcrModel(*M.bcr_blocks(sysS, K))
        _discriminates(model, "S", y, tol, padded(y, model.ns[0]))
    for sysE in M.gpu_band_systems(N, l, u, np.float64)[1]:
        model = M.BcrModel(*M.bcr_blocks(sysE, K))
        _discriminates(model, "E", None, 0.0, padded(sysE.y.astype(np.float64), model.ns[0]))


@pytest.mark.parametrize("nb,bs", M.BLOCK_SHAPES)
def test_block_cases_discriminate_at_every_level(nb, bs):
    q = M.BLOCK_SHAPES.index((nb, bs))
    fams = [("dom", lambda nb, bs, lam, seed, dtype: M.gpu_block_systems(nb, bs, dtype)[0], 0)]
    if (nb, bs) in M.BLOCK_DENSE_SHAPES:
        fams.append(("dense", M.s_block_dense, 73 + M.BLOCK_DENSE_SHAPES.index((nb, bs))))
    for dtype in (np.float64, np.float32):
        for _name, fam, seed in fams:
            s = fam(nb, bs, M.block_lam(nb), seed, dtype)
            y, tol = _s_ref(s, dtype)
            _discriminates(M.BcrModel(*M.bcr_blocks(s, bs)), "S", None, tol, y.reshape(nb, bs))
    for s in M.gpu_block_systems(nb, bs, np.float64)[1]:
        _discriminates(M.BcrModel(*M.bcr_blocks(s, bs)), "E", None, 0.0, s.y.astype(np.float64).reshape(nb, bs))


def test_every_level_the_solvers_have_is_covered():
    # the GPU lists reach the deepest schedules: 6 tridiagonal levels (10^7 rows: 5 reductions and the top), banded levels on both sides of kBcrTopRows
    assert max(len(M.tri_levels(N)) for N in M.TRI_E_N) == len(M.tri_levels(10 ** 7)) == 6
    tops = {(-(-N // M.band_K(l, u))) for N, l, u in M.BAND_SHAPES}
    assert {M.BCR_TOP_ROWS, M.BCR_TOP_ROWS + 1, 2 * M.BCR_TOP_ROWS, 2 * M.BCR_TOP_ROWS + 1} <= tops


# ------------------------------------------------------------------------------------------------------------ the old inputs are blind
def _reach(Ainv_col, j, thresh):
    far = np.flatnonzero(np.abs(Ainv_col) > thresh)
    return int(np.max(np.abs(far - j)))


def test_the_older_tridiagonal_inputs_do_not_see_the_upper_levels():
    N = 40000
    dl, d, du, b, alpha, beta = SI.tridiag_system(N, 100 + N)
    a = np.concatenate([[0.0], beta * dl]); c = np.concatenate([beta * du, [0.0]]); bb = alpha + beta * d
    want = SI.tridiag_reference(dl, d, du, b, alpha, beta)
    e = np.zeros(N); e[N // 2] = 1.0
    col = SI.tridiag_reference(dl, d, du, e, alpha, beta)
    reach11, reach16 = _reach(col, N // 2, 1e-11), _reach(col, N // 2, 1e-16)
    assert 9 / 2 <= reach11 <= 9 * 2 and 12 / 2 <= reach16 <= 12 * 2, (reach11, reach16)
    model = M.TriModel(a, bb, c, b)
    assert len(model.ns) >= 4
    tol = 1e-11 * max(1.0, np.max(np.abs(want)))
    assert np.max(np.abs(model.solve() - want)) <= tol
    for L in model.fault_levels:
        for mode in MODES:
            err = np.max(np.abs(model.with_fault(L, mode).solve() - want))
            assert (err <= tol) == (L >= 2), (L, mode, err)           # level 1 (rows 8 apart) is the last one their assertion sees


@pytest.mark.parametrize("l,u,reach", [(1, 2, 8), (2, 2, 15), (4, 4, 29)])
def test_the_older_banded_inputs_do_not_see_the_upper_levels(l, u, reach):
    N, gamma = 6000, SI.BAND_GAMMA
    rng = np.random.default_rng(N + 10 * l + u)
    data = SI.band(N, l, u, rng)
    b = rng.standard_normal(N)
    want = SI.band_scipy_solve(data, N, l, u, 1.0, -gamma, b)
    e = np.zeros(N); e[N // 2] = 1.0
    got = _reach(SI.band_scipy_solve(data, N, l, u, 1.0, -gamma, e), N // 2, 1e-11)
    assert reach / 2 <= got <= reach * 2, got
    i = np.arange(N)
    A = {k: np.where((i + k >= 0) & (i + k < N), -gamma * data[u - k, np.clip(i + k, 0, N - 1)], 0.0) for k in range(-l, u + 1)}
    A[0] = 1.0 + A[0]
    K = M.band_K(l, u)
    model = M.BcrModel(*M.bcr_blocks(M.System("band", N, 1.0, -gamma, data, b, A, None, {}), K))
    tol = 1e-11 * max(1.0, np.max(np.abs(want)))
    assert np.max(np.abs(model.solve().reshape(-1)[:N] - want)) <= tol
    blind_from = int(np.ceil(np.log2(2.0 * got / K))) + 1           # block rows 2^L apart, beyond twice the reach
    assert blind_from <= 5 and blind_from < max(model.fault_levels)
    for L in model.fault_levels:
        if L >= blind_from:
            for mode in MODES:
                assert np.max(np.abs(model.with_fault(L, mode).solve().reshape(-1)[:N] - want)) <= tol, (L, mode)


def test_the_older_block_inputs_do_not_see_the_upper_levels():
    nb, bs = 200, 32
    data, rhs, gamma = SI.block_system(nb, bs, 2 * 2 * bs * bs + (nb - 2) * 3 * bs * bs)       # (the layout's data_len for nb >= 2)
    A = M.block_seen(data, nb, bs, 1.0, -gamma)
    s = M.System("block", nb * bs, 1.0, -gamma, data, rhs, A, None, {})
    solve = M.lapack_solver(A, s.N)
    want = solve(rhs)
    e = np.zeros(s.N); e[(nb // 2) * bs] = 1.0
    got = _reach(solve(e), (nb // 2) * bs, 1e-11) / bs
    assert 5 / 2 <= got <= 5 * 2, got
    model = M.BcrModel(*M.bcr_blocks(s, bs))
    tol = 1e-11 * max(1.0, np.max(np.abs(want)))
    assert np.max(np.abs(model.solve().reshape(-1) - want)) <= tol
    blind_from = int(np.ceil(np.log2(2.0 * got))) + 1
    assert blind_from <= 5 and blind_from < max(model.fault_levels)
    for L in model.fault_levels:
        if L >= blind_from:
            for mode in MODES:
                assert np.max(np.abs(model.with_fault(L, mode).solve().reshape(-1) - want)) <= tol, (L, mode)
