"""The pair model of the complex step (tests/exact_model.py: c_mul, c_smul, ..., fixture_complex, colour_values_complex) and the cases
of tests/exact_complex_cases.py, on the CPU: nothing here loads libfdjac or torch (the cases take their stencil patterns from the package's pure-numpy
patterns module, as tests/exact_general.py does).

  * the linear families against exact rational arithmetic: every stored value IS the stencil coefficient, bit for bit
  * every GPU case evaluated with the model alone; the finite share of its stored values (MIN_FINITE; nan_inf exempt)
  * `re_overflow` overflows the REAL part in most rows and keeps every stored value finite
  * the cases discriminate: two named mutations of the model each change stored bits of a named case
  * a case's inputs are built from its name alone
  * the block-coupled residual: the C oracle meets the per-entry bound of tests/blockcoupled_bound.py against mpmath (worst ratio to the
    bound 0.24, at (nb, bs) = (9, 64) in Float64), and the bound sees a fault the global tolerance 1e-12 max|J| cannot"""
from fractions import Fraction

import numpy as np
import pytest

import exact_complex_cases as Z
import exact_model as X

_MODEL = {}


def _model(case):
    k = Z.model_key(case)
    if k not in _MODEL:
        _MODEL[k] = Z.model(case)
    return _MODEL[k]


def _case(cid):
    return next(c for c in Z.CASES if c["id"] == cid)


def test_pair_operators_one_ieee_operation_each():
    a = (np.array([1.5, np.inf, -0.0, 3.0]), np.array([0.25, 0.0, 0.0, -2.0]))
    b = (np.array([2.0, 1.0, 5.0, 0.5]), np.array([-1.0, 0.0, -0.0, 4.0]))
    with np.errstate(all="ignore"):
        re, im = X.c_mul(a, b)
        assert np.array_equal(re[[0, 3]], [1.5 * 2.0 - 0.25 * -1.0, 3.0 * 0.5 - -2.0 * 4.0])
        assert np.array_equal(im[[0, 3]], [1.5 * -1.0 + 0.25 * 2.0, 3.0 * 4.0 + -2.0 * 0.5])
        assert re[1] == np.inf and np.isnan(im[1])                   # (Inf, 0) (1, 0): Inf 0 in the imaginary part
        sre, sim = X.c_smul(np.float64(2.0), a)
        assert sre[1] == np.inf and sim[1] == 0.0 and not np.signbit(sim[1])      # scalar * complex: component-wise, no NaN
        assert np.signbit(sre[2]) and not np.signbit(sim[2])
        assert np.array_equal(X.c_add_s(a, 1.0)[1], a[1]) and np.array_equal(X.c_sub_s(a, 1.0)[1], a[1])
        assert np.array_equal(X.c_div_s(a, 2.0)[1], a[1] / 2.0)
        assert np.array_equal(X.c_sub(a, b)[1], a[1] - b[1]) and np.array_equal(X.c_add(a, b)[0], a[0] + b[0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fixture,shape,col", [("tridiag", (129,), "cyc3_0"), ("lap5", (6, 5), "stencil")])
def test_linear_families_store_the_exact_coefficients(fixture, shape, col, dtype):
    # exact rational arithmetic: im(f(x + i e m_c)) = e * (coefficient), a power of two times a small integer -- no rounding anywhere,
    # so the quotient by e is the coefficient itself whatever the (ordinary) real parts are
    case = Z._case("handover", fixture, shape, col, "f64" if dtype == np.float64 else "f32")
    inp = Z.inputs(case)
    (got,), eps = Z.model(case)
    assert (eps == np.finfo(dtype).eps).all() and eps.dtype == dtype
    rows = inp["rowval"] - 1
    cols = np.repeat(np.arange(inp["N"]), np.diff(inp["colptr"]))
    centre = Fraction(-2) if fixture == "tridiag" else Fraction(-4)
    e = Fraction(float(eps[0]))
    want = np.array([float((e * (centre if r == j else Fraction(1))) / e) for r, j in zip(rows, cols)], dtype=dtype)
    assert X.same_bits(got, want).all()
    assert got.dtype == dtype


@pytest.mark.parametrize("case", Z.CASES, ids=[c["id"] for c in Z.CASES])
def test_every_gpu_case_is_computable_by_the_model_alone(case):
    lay, eps = _model(case)
    inp = Z.inputs(case)
    assert eps.dtype == inp["dtype"] and (eps == np.finfo(inp["dtype"]).eps).all() and eps.size == inp["C"]
    vals = np.concatenate([np.asarray(a).reshape(-1) for a in lay])
    assert vals.dtype == inp["dtype"]
    if case["dest"] == "dense":         # (the share is taken over the pattern's entries: a dense J is mostly structural zeros)
        D = X.colour_values_complex(inp["f"], inp["x"], inp["c0"], inp["C"], eps)
        vals = X.to_csc(D, inp["c0"], inp["colptr"], inp["rowval"])
    if case["family"] != "nan_inf" and vals.size:
        assert np.isfinite(vals).mean() >= Z.MIN_FINITE, (case["id"], float(np.isfinite(vals).mean()))
    if case["family"] == "re_overflow" and case["fixture"] not in ("tridiag", "lap5"):      # (the linear families have no product to overflow)
        with np.errstate(all="ignore"):
            re, _im = inp["f"]((inp["x"], np.where(inp["c0"] == 0, eps[0], 0).astype(inp["dtype"])))
        assert np.isinf(re).mean() + np.isnan(re).mean() > 0.5, (case["id"], float(np.isinf(re).mean()))
        assert np.isfinite(vals).all(), case["id"]
    if case["family"] == "f32_im_subnormal":
        assert (np.abs(inp["x"][inp["x"] != 0]) * eps[0] < np.finfo(np.float32).tiny).all()       # x eps is a subnormal


def test_the_table_covers_every_route_and_family():
    seen = {(c["route"], c["dtype"], c["family"]) for c in Z.CASES}
    for fam in Z.FAMILIES64:
        for route in ("handover", "lazy", "cols", "jit", "terms"):
            assert (route, "f64", fam) in seen, (route, fam)
    for fam in Z.FAMILIES32:
        for route in ("handover", "lazy", "cols", "jit", "terms"):
            assert (route, "f32", fam) in seen, (route, fam)
    fixtures = {c["fixture"] for c in Z.CASES if c["route"] == "handover"}
    assert fixtures == {"tridiag", "tridiag_nl", "lap5", "lap5_nl", "lap7", "sparse"}
    assert {c["dest"] for c in Z.CASES if c["route"] == "handover"} == {"csc_list", "csc_window", "banded", "tridiagonal", "dense", "colwindow", "colorrange"}
    assert {c["shape"][0] for c in Z.CASES if c["fixture"].startswith("tridiag")} >= set(Z.TRIDIAG_SIZES) | {Z.TRIDIAG_OPERAND_N}
    assert {c["shape"] for c in Z.CASES if c["fixture"].startswith("lap5")} >= set(Z.LAP5_GRIDS) | {Z.LAP5_OPERAND_GRID}
    counts = {}
    for c in Z.CASES:
        counts[(c["route"], c["dtype"])] = counts.get((c["route"], c["dtype"]), 0) + 1
    print("\ncomplex-step cases per route and element type:", sorted(counts.items()))


def _full_product(s, a):
    """The mutation: scalar * complex widened to the complex product (s, 0) (ar, ai)."""
    s = np.zeros_like(a[0]) + s
    return X.c_mul((s, np.zeros_like(s)), a)


MUTATION_SMUL_CASES = ["handover-tridiag-1025-ones-f64-nan_inf-csc_list"] + [c["id"] for c in Z.CASES if c["fixture"] == "tridiag" and
                                                                              c["family"] == "nan_inf" and c["shape"] == (Z.TRIDIAG_OPERAND_N,)]


@pytest.mark.parametrize("cid", MUTATION_SMUL_CASES)
def test_mutation_full_product_for_scalar_times_complex_is_seen(cid):
    # 2 * (Inf, 0): component-wise (Inf, 0); as a complex product the imaginary part is 2 * 0 + 0 * Inf = NaN.  The linear rows next to an
    # Inf coordinate store their coefficient under the device's arithmetic and NaN under the mutation.
    case = _case(cid)
    good, _ = _model(case)
    bad, _ = Z.model(case, smul=_full_product)
    diff = sum(int((~X.same_bits(g, b)).sum()) for g, b in zip(good, bad))
    assert diff >= 1, cid
    # ... and only there: with ordinary operands the two products agree bit for bit
    ordinary = _case("handover-tridiag_nl-513-none-f64-ordinary-csc_list")
    g2, _ = _model(ordinary)
    b2, _ = Z.model(ordinary, smul=_full_product)
    assert all(X.same_bits(g, b).all() for g, b in zip(g2, b2))


MUTATION_POINT_CASES = ["handover-sparse-random_band600-invalid6-f64-ordinary-dense", "handover-tridiag_nl-513-ones-f64-ordinary-csc_list",
                        "cols-sparse-tiny_2-ones-f32-ordinary-csc_list"]


def _column_point_values(inp, eps):
    """The mutation: every stored entry (r, j) from the COLUMN's point x + i eps e_j instead of the colour's."""
    cp = inp["colptr"] - 1
    out = np.zeros(inp["rowval"].size, inp["dtype"])
    T = inp["dtype"]
    with np.errstate(all="ignore"):
        for j in range(inp["N"]):
            if inp["c0"][j] < 0 or cp[j] == cp[j + 1]:
                continue
            e = T(eps[inp["c0"][j]])
            im = np.zeros(inp["N"], T)
            im[j] = e
            _re, fi = inp["f"]((inp["x"], im))
            out[cp[j]:cp[j + 1]] = fi[inp["rowval"][cp[j]:cp[j + 1]] - 1] / e
    return out


@pytest.mark.parametrize("cid", MUTATION_POINT_CASES)
def test_mutation_column_point_under_an_invalid_colouring_is_seen(cid):
    case = _case(cid)
    inp = Z.inputs(case)
    eps = X.complex_epsilons(inp["C"], inp["dtype"])
    D = X.colour_values_complex(inp["f"], inp["x"], inp["c0"], inp["C"], eps)
    good = X.to_csc(D, inp["c0"], inp["colptr"], inp["rowval"])
    bad = _column_point_values(inp, eps)
    assert int((~X.same_bits(good, bad)).sum()) >= 1, cid


def test_column_point_equals_colour_point_under_a_valid_colouring():
    # (what lets the column stores take the column's point when the plan has verified the colouring)
    case = _case("handover-sparse-random_band600-greedy-f64-ordinary-dense")
    inp = Z.inputs(case)
    eps = X.complex_epsilons(inp["C"], inp["dtype"])
    D = X.colour_values_complex(inp["f"], inp["x"], inp["c0"], inp["C"], eps)
    assert X.same_bits(X.to_csc(D, inp["c0"], inp["colptr"], inp["rowval"]), _column_point_values(inp, eps)).all()


def test_inputs_are_built_from_the_name_alone():
    ids = [c["id"] for c in Z.CASES]
    assert len(set(ids)) == len(ids)
    for case in Z.CASES[::7]:
        again = Z._case(case["route"], case["fixture"], case["shape"], case["colouring"], case["dtype"], case["family"], case["dest"], case["imag_only"])
        assert again == case
        a, b = Z.inputs(case), Z.inputs(again)
        assert X.same_bits(a["x"], b["x"]).all() and np.array_equal(a["colors"], b["colors"]) and np.array_equal(a["rowval"], b["rowval"])


def test_the_cases_reach_signed_zero_coordinates_and_stored_zeros():
    # the unperturbed imaginary part is +0, so a stored zero's sign comes out of the arithmetic alone: the linear 5-point rows under the
    # `ones` colouring cancel to (e + e + e + e) - 4 e = +0 in the interior, and columns without a colour hold +0
    case = _case("handover-tridiag_nl-1025-ones-f64-signed_zeros-csc_list")
    inp = Z.inputs(case)
    assert np.signbit(inp["x"][inp["x"] == 0]).any() and (~np.signbit(inp["x"][inp["x"] == 0])).any()
    (vals,), _ = _model(_case("handover-lap5-70x40-ones-f32-f32_im_subnormal-csc_list"))
    assert (vals == 0).mean() > 0.5 and not np.signbit(vals[vals == 0]).any()
    (vals,), _ = _model(_case("handover-sparse-random_band-none5-f64-ordinary-csc_list"))
    assert (vals == 0).any() and not np.signbit(vals[vals == 0]).any()


# ---- the block-coupled residual: a per-entry bound against mpmath (tests/blockcoupled_bound.py) ------------------------------------------
import blockcoupled_bound as BB

ORACLE_RATIOS = {}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", BB.SHAPES, ids=["%dx%d" % s for s in BB.SHAPES])
def test_blockcoupled_oracle_meets_the_per_entry_bound(oracle, shape, dtype):
    # the C oracle (its own summation order, libm's csin) against the mpmath value of every entry: inside the bound derived for the device
    nb, bs = shape
    lay = BB.layout(nb, bs)
    x = BB.operands(nb, bs, dtype)
    ref = oracle.jacobian("complex", oracle.Fixture("blockcoupled", nb, bs, dtype=dtype), x, lay.colors(), kind=oracle.PAT_BLOCKBANDED,
                          blk_sizes=lay.blk_sizes, bl=1, bu=1, block_starts=lay.block_starts, block_strides=lay.block_strides,
                          out_len=lay.data_len)
    out = np.asarray(ref["out"])
    assert out.dtype == dtype
    ratio, at = BB.worst_ratio(lay.to_dense(out), nb, bs, dtype)
    ORACLE_RATIOS[(shape, np.dtype(dtype).name)] = ratio
    print("\nblock-coupled oracle, %s %s: worst error / bound = %.4f at %s" % (shape, np.dtype(dtype).name, ratio, at))
    assert ratio <= 1.0, (shape, ratio, at)


def test_blockcoupled_bound_is_tight_enough_to_see_a_wrong_entry():
    # one ulp-level fault the old global tolerance 1e-12 max|J| cannot see: a small off-diagonal entry off by 1e-9 of itself
    nb, bs = 5, 32
    hi, _lo = BB.reference(nb, bs, np.float64)
    B = BB.bound(nb, bs, np.float64)
    m = BB.band_mask(nb, bs)
    assert (B[m] > 0).all() and (B[m] <= 40 * np.finfo(np.float64).eps * (np.abs(hi[m]) + 3 * bs)).all()
    k, j = np.unravel_index(np.argmin(np.where(m & (hi != 0), np.abs(hi), np.inf)), hi.shape)
    bad = hi.copy()
    bad[k, j] *= 1 + 1e-9
    assert abs(bad[k, j] - hi[k, j]) < 1e-12 * np.abs(hi).max()         # invisible to the global tolerance
    assert BB.worst_ratio(bad, nb, bs, np.float64)[0] > 1e5              # far outside the entry's own bound
    assert BB.worst_ratio(hi, nb, bs, np.float64)[0] <= 1.0              # the rounded reference itself: half an ulp
