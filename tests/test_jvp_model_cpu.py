"""The exact host model of the finite-difference JVP (tests/jvp_model.py) and its cases (tests/jvp_cases.py) on the CPU: the three
summation orders against the exact sum within a derived bound, the grid's restatement, every GPU case's inputs through the model (finite
shares, finite non-zero step sizes, the all_nan rule), and that the cases can tell the model from its plausible neighbours -- another
summation order, a cast after the sqrt, fused points, dir in the central rule, a plain max, f_in in the central arm, a reciprocal."""
import collections
import fractions

import numpy as np
import pytest

import exact_model as X
import jvp_cases as C
import jvp_model as J

Fr = fractions.Fraction
ORDERS = ("small", "scalar", "paired")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _exact_dot(x, v):
    """(sum x_i v_i, sum |x_i v_i|) as exact rationals: integer significands, one common power of two."""
    mx, ex = np.frexp(x.astype(np.float64))
    mv, ev = np.frexp(v.astype(np.float64))
    ix, iv = (mx * 2.0 ** 53).astype(np.int64), (mv * 2.0 ** 53).astype(np.int64)      # exact: |m| < 1 has 53 bits
    e = ex.astype(np.int64) + ev.astype(np.int64)
    e0 = int(e.min())
    tot = mag = 0
    for a, b, k in zip(ix.tolist(), iv.tolist(), (e - e0).tolist()):
        p = (a * b) << k
        tot += p
        mag += abs(p)
    scale = Fr(2) ** (e0 - 106)
    return tot * scale, mag * scale


@pytest.mark.parametrize("num_cus", [1, 104, 256, 304])
def test_balanced_grid_restatement(num_cus):
    """Against the definition (the fewest whole rounds of at most 8 num_cus workgroups, then the fewest workgroups that cover the
    tiles in that many rounds) by search, and at hand-computed values."""
    cap = 8 * num_cus
    for n in C.SIZES + (256, 524288, 524289, 10 ** 7):
        tiles = -(-n // 256)
        rounds = next(r for r in range(1, tiles + 1) if r * cap >= tiles)
        want = next(g for g in range(1, cap + 1) if g * rounds >= tiles)
        assert J.grid(n, num_cus) == want, (n, num_cus)
        assert want <= cap and (want == tiles or rounds > 1)
    by_hand = {1: (8, 8), 104: (157, 782), 256: (157, 1172), 304: (157, 2344)}      # N = 40001 (157 tiles), 600001 (2344 tiles)
    assert (J.grid(40001, num_cus), J.grid(600001, num_cus)) == by_hand[num_cus]
    assert J.balanced_grid(4883, 2048) == 1628 and J.balanced_grid(0, 0) == 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", C.SIZES)
def test_dot_orders_against_the_exact_sum(n, dtype):
    """|dot - sum x_i v_i| <= (L + 1) u sum |x_i v_i| with L the order's longest chain of additions (jvp_model.chain_length), + 1 for
    the product's own rounding, u = 2^-53: the first-order bound of any summation whose terms each pass through at most L additions
    (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  Exact rational arithmetic on both sides."""
    rng = np.random.default_rng(n)
    x = (rng.random(n) - 0.5).astype(dtype)
    v = ((rng.random(n) - 0.5) * 10.0 ** rng.integers(-3, 4, n)).astype(dtype)
    exact, mag = _exact_dot(x, v)
    for num_cus in (256, 1) if n != 600001 else (256,):
        for order in ORDERS:
            t = J.dot(x, v, order, num_cus)
            L = J.chain_length(order, n, num_cus)
            assert abs(Fr(float(t)) - exact) <= (L + 1) * Fr(J.U) * mag, (order, n, num_cus, L)
    # the three orders are the same sum where they must be: one term per thread, all within the first wave's tree
    if n <= 64:
        assert J.dot(x, v, "small") == J.dot(x, v, "scalar", 256)


def test_dot_orders_at_hand_worked_sizes():
    """Sums worked out by hand with B = 2^53 (B + 1 rounds back to B, 1 + 1 + B is B + 2): where a term sits decides the result.
    n = 3, x = (1, 1, B): the paired order's thread 0 holds (1 + 1), then the tail B -> B + 2; the scalar and the small order hold one
    term per lane, lane 0 takes lane 2 first (1 + B = B), then lane 1 (B + 1 = B).
    n = 2050 on ONE CU (9 tiles, cap 8 -> 2 rounds -> 5 workgroups, 1280 threads), x_0 = x_1280 = 1, x_1 = B: the scalar order's thread
    0 holds 1 + 1 and meets lane 1's B in the tree -> B + 2; the small order has x_1280 on thread 256 (wave 4): (1 + B) + 1 = B; the
    paired order has (x_0, x_1) on thread 0 and x_1280 on thread 640 (workgroup 2): B and 1 meet in k_jvp_eps's tree -> B."""
    B = 2.0 ** 53
    x, v = np.array([1.0, 1.0, B]), np.ones(3)
    assert J.dot(x, v, "paired", 256) == B + 2 and J.dot(x, v, "scalar", 256) == B and J.dot(x, v, "small") == B
    x, v = np.zeros(2050), np.ones(2050)
    x[0], x[1280], x[1] = 1.0, 1.0, B
    assert J.grid(2050, 1) == 5
    assert J.dot(x, v, "scalar", 1) == B + 2 and J.dot(x, v, "small") == B and J.dot(x, v, "paired", 1) == B
    # every accumulator starts from +0.0: a lone -0 product sums to +0
    for order in ORDERS:
        assert J.dot(np.array([-0.0]), np.array([1.0]), order).tobytes() == np.float64(0.0).tobytes()
        assert J.dot(np.array([-0.0, -0.0, -0.0], np.float32), np.array([1.0, 2.0, 3.0], np.float32), order).tobytes() == np.float64(0.0).tobytes()


def test_epsilon_rule_and_defaults():
    for dtype in (np.float64, np.float32):
        T = np.dtype(dtype).type
        e = np.finfo(dtype).eps
        assert J.steps("forward", None, None, dtype) == (float(np.sqrt(T(e))), float(np.sqrt(T(e))))
        assert J.steps("central", -1.0, -1.0, dtype) == (float(np.cbrt(T(e))), float(np.cbrt(T(e))))
        assert J.steps("forward", 0.0, 0.0, dtype)[1] == 0.0 and J.steps("forward", 1e-3, -1.0, dtype) == (1e-3, 1e-3)
        assert J.epsilon(0.0, "forward", dtype=dtype) == T(np.sqrt(T(e))) and J.epsilon(0.0, "forward", absstep=0.0, dtype=dtype) == 0
        assert J.epsilon(-4.0, "forward", 0.5, 0.25, -1.0, dtype) == T(-1.0) and J.epsilon(-4.0, "central", 0.5, 0.25, -1.0, dtype) == T(1.0)
        assert J.epsilon(4.0, "central", 0.5, 8.0, dtype=dtype) == T(8.0)
        assert np.isnan(J.epsilon(np.nan, "forward", dtype=dtype)) and J.epsilon(np.inf, "central", dtype=dtype) == np.inf
        assert J.epsilon(1e300, "forward", dtype=dtype) == (np.inf if dtype == np.float32 else T(np.sqrt(e)) * T(1e150))
        assert type(J.epsilon(2.0, "forward", dtype=dtype)) is T


def test_jvp_arms_on_a_linear_fixture():
    f = X.fixture("tridiag")
    x, v = np.array([1.0, 2.0, 4.0]), np.array([1.0, 0.0, -1.0])
    Jv = np.array([-2.0, 0.0, 2.0])                        # tridiag(1, -2, 1) v; eps = 2^-10: every operation is exact
    for fdtype in ("forward", "central"):
        assert np.array_equal(J.jvp(f, x, v, 2.0 ** -10, fdtype), Jv)
    assert np.array_equal(J.jvp(f, x, v, 0.5, "forward", f_in=np.zeros(3)), f(x + 0.5 * v) / 0.5)
    assert np.array_equal(J.jvp(f, x, v, 0.5, "central", f_in=np.zeros(3)), Jv)
    assert J.jvp(f, x.astype(np.float32), v.astype(np.float32), 0.5, "central").dtype == np.float32


@pytest.fixture(scope="module")
def answers():
    """{case id: (want, eps, t)} of every case, each distinct model answer computed once."""
    memo, out = {}, {}
    for c in C.CASES:
        key = (c["family"], c["prm"], c["dtype"], c["fdtype"], c["ops"], c["f_in"], c["dir"], C.dot_order(c), c["form"] == "reuse")
        if key not in memo:
            memo[key] = C.model(c)
        out[c["id"]] = memo[key]
    return out


def test_every_case_keeps_its_finite_share(answers):
    bad = []
    nan_slots = collections.Counter()
    for c in C.CASES:
        M, N = C.shape(c)
        want, eps, _t = answers[c["id"]]
        assert want.shape == (M,) and want.dtype == C.np_dtype(c) and type(eps) is np.dtype(C.np_dtype(c)).type, c["id"]
        calls = [(want, eps)] + ([C.model(c, call=1)[:2]] if c["form"] == "reuse" else [])
        for w, e in calls:
            if c["all_nan"]:
                if not np.isnan(w).all():
                    bad.append((c["id"], "not every value is NaN"))
            elif np.isfinite(w).mean() < C.MIN_FINITE or not np.isfinite(e) or e == 0:
                bad.append((c["id"], float(np.isfinite(w).mean()), float(e)))
        if c["all_nan"]:
            assert c["ops"] in C.ALL_NAN and c["family"] == "tridiag_nl", c["id"]
            nan_slots[(C.route(c), c["dtype"])] += 1
        if c["form"] == "reuse":                           # a stale step size or partial would show: the second call's differ
            assert _bits(calls[0][1]) != _bits(calls[1][1]) and not np.array_equal(calls[0][0], calls[1][0]), c["id"]
    assert not bad, bad
    assert max(nan_slots.values()) == 1, nan_slots
    assert {c["ops"] for c in C.CASES if c["all_nan"]} == set(C.ALL_NAN)


def test_case_table_covers_what_it_claims():
    by = collections.Counter((C.route(c), c["dtype"]) for c in C.CASES)
    for r in ("small", "mat_paired", "mat_scalar", "lazy_values", "lazy_quotient", "declined"):
        assert by[(r, "f64")] >= 3 and by[(r, "f32")] >= 3, (r, by)
    fams = collections.defaultdict(set)
    for c in C.CASES:
        fams[(c["family"], c["dtype"])].add(C.route(c))
    for fam in ("tridiag", "tridiag_nl", "lap5", "lap5_nl"):
        for dt in ("f64", "f32"):
            assert fams[(fam, dt)] >= {"small", "mat_paired", "mat_scalar", "lazy_values", "lazy_quotient"}, (fam, dt)
    for dt in ("f64", "f32"):
        assert fams[("sparse", dt)] >= {"small", "mat_paired", "mat_scalar"}
    default = {C.shape(c)[1] for c in C.CASES if c["family"].startswith("tridiag") and not c["small_off"] and c["form"] == "device"
               and c["lazy"] and c["quotient"] and not c["xoff"] and not c["outoff"] and c["dtype"] == "f64"}
    assert default >= set(C.SIZES)
    assert {C.shape(c)[1] for c in C.CASES if c["small_off"] and c["family"].startswith("tridiag")} >= set(C.SMALL_OFF_SIZES)
    shapes = {C.shape(c) for c in C.CASES if c["family"] == "sparse"}
    assert any(M == 1 for M, N in shapes) and any(M % 2 == 1 and M > 1 and M != N for M, N in shapes) and any(M > N for M, N in shapes)
    assert {c["form"] for c in C.CASES} == {"device", "host", "async", "reuse"}
    assert {c["ops"] for c in C.CASES} == set(C.OPERANDS)
    assert any(c["dir"] < 0 and c["fdtype"] == f for c in C.CASES for f in ("forward",)) and any(c["dir"] < 0 and c["fdtype"] == "central" for c in C.CASES)
    # two grid rounds at 256 CUs
    assert 600001 > J.grid(600001, 256) * 256 and J.grid(600001, 256) < -(-600001 // 256)


# ---- the perturbed models ------------------------------------------------------------------------------------------------------------
def _fused_points(x, e, v, sign):
    """x + sign (e v) with ONE rounding.  Float64: exact rationals, correctly rounded by float(); Float32: in Float64 (the product is
    exact there), then rounded -- a double rounding in rare ties, which a perturbed model may have."""
    if x.dtype == np.float32:
        return (x.astype(np.float64) + sign * (np.float64(e) * v.astype(np.float64))).astype(np.float32)
    plain = x + sign * (e * v)
    out = np.array([float(Fr(float(a)) + sign * Fr(float(e)) * Fr(float(b))) for a, b in zip(x, v)])
    return np.where(out == 0, plain, out)                  # (the sign of an exact zero: as the plain sum's)


def _jvp_fma(f, x, v, eps, fdtype, f_in=None):
    T = x.dtype.type
    with np.errstate(all="ignore"):
        e = T(eps)
        if fdtype == "forward":
            base = f(x) if f_in is None else np.asarray(f_in, dtype=x.dtype)
            return (f(_fused_points(x, e, v, 1)) - base) / e
        return (f(_fused_points(x, e, v, 1)) - f(_fused_points(x, e, v, -1))) / (T(2) * e)


def _jvp_f_in_central(f, x, v, eps, fdtype, f_in=None):
    if fdtype == "forward" or f_in is None:
        return J.jvp(f, x, v, eps, fdtype, f_in)
    T = x.dtype.type
    with np.errstate(all="ignore"):
        return (f(x + T(eps) * v) - np.asarray(f_in, dtype=x.dtype)) / (T(2) * T(eps))


def _jvp_reciprocal(f, x, v, eps, fdtype, f_in=None):
    T = x.dtype.type
    with np.errstate(all="ignore"):
        e = T(eps)
        ev = e * v
        if fdtype == "forward":
            base = f(x) if f_in is None else np.asarray(f_in, dtype=x.dtype)
            return (f(x + ev) - base) * (T(1) / e)
        return (f(x + ev) - f(x - ev)) * (T(1) / (T(2) * e))


def _eps_dir_central(t, fdtype, relstep=None, absstep=None, dir=1.0, dtype=np.float64):
    return J.epsilon(t, fdtype, relstep, absstep, dir, dtype, dir_in_central=True)


def _eps_plain_max(t, fdtype, relstep=None, absstep=None, dir=1.0, dtype=np.float64):
    return J.epsilon(t, fdtype, relstep, absstep, dir, dtype, max_=lambda a, b: a if a > b else b)


def _changed(answers, cases, **kw):
    """How many of `cases` change a bit of their values / of their step size under the perturbed model."""
    vals = eps = 0
    for c in cases:
        want, e0, _t = answers[c["id"]]
        got, e1, _t1 = C.model(c, **kw)
        vals += int(not X.same_bits(got, want).all())
        eps += int(not X.same_bits(np.array(e1), np.array(e0)).all())
    return vals, eps


def test_the_cases_tell_the_models_apart(answers):
    """Counts (cases whose bits change / cases tried) are printed: run with -s to see them."""
    report = {}
    f64 = [c for c in C.CASES if c["dtype"] == "f64" and not c["all_nan"]]
    # another summation order: the STEP SIZE differs, not only the dot product
    for a, b in (("small", "scalar"), ("small", "paired"), ("scalar", "paired")):
        n = tried = 0
        for c in f64:
            if C.dot_order(c) not in (a, b) or c["ops"] != "generic":
                continue
            tried += 1
            inp = C.inputs(c)
            ea, eb = (J.epsilon(J.dot(inp["x"], inp["v"], o), c["fdtype"], inp["rel"], inp["ab"], inp["dir"]) for o in (a, b))
            n += int(_bits(ea) != _bits(eb))
        report["eps %s / %s" % (a, b)] = (n, tried)
        assert n >= 1, (a, b)
    # Float32: the cast comes BEFORE the sqrt
    f32 = [c for c in C.CASES if c["dtype"] == "f32" and not c["all_nan"]]
    with np.errstate(all="ignore"):
        n = sum(int(np.sqrt(np.abs(np.float32(answers[c["id"]][2]))) != np.float32(np.sqrt(np.abs(answers[c["id"]][2])))) for c in f32)
    report["sqrt(T(t)) != T(sqrt(t))"] = (n, len(f32))
    assert n >= 1
    live = [c for c in C.CASES if c["form"] != "reuse"]
    small = [c for c in live if C.shape(c)[1] <= 1100 and not c["all_nan"]]             # (the exact fused points are slow)
    central = [c for c in live if c["fdtype"] == "central"]
    for name, cases, kw in (("fused points", small, dict(jvp=_jvp_fma)), ("dir in the central rule", central, dict(epsilon=_eps_dir_central)),
                            ("plain max", live, dict(epsilon=_eps_plain_max)), ("f_in in the central arm", central, dict(jvp=_jvp_f_in_central)),
                            ("reciprocal", live, dict(jvp=_jvp_reciprocal))):
        vals, eps = _changed(answers, cases, **kw)
        report[name] = (vals, eps, len(cases))
        assert vals >= 1, name
    for k, v in report.items():
        print("%-28s %s" % (k, v))
