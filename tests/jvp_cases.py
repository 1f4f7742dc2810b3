"""The cases of tests/test_gpu_exact_jvp.py: the finite-difference JVP on every route against the exact host model
(tests/jvp_model.py).  Pure numpy -- shapes, operands, the table of cases, which route a case takes and the model's answer -- so that
the CPU suite (tests/test_jvp_model_cpu.py) can evaluate every GPU case's inputs with the model alone.  Test infrastructure only.

  route     which kernels a case reaches (jvp_enqueue's own rule, restated in route()):
              small          N <= 16384 without FDJAC_SMALL=0: k_jvp_small
              mat_paired     k_dot_partial<true> + k_jvp_eps + k_jvp_points<true>          (x, v aligned to a pair)
              mat_scalar     k_dot_partial<false> + k_jvp_eps + k_jvp_points<false>        (x, v offset by one element)
              lazy_values    dot + k_jvp_eps, the family's lazy launcher writes f's values, k_jvp_diff
              lazy_quotient  dot + k_jvp_eps, the family's lazy launcher writes the finished quotient
              declined       dot + k_jvp_eps, a launcher that returns FD_LAZY_DECLINED, then the materialised points
            `xoff` / `outoff` offset x and v / out by one element (outoff: the scalar k_jvp_diff, and no quotient from a lazy launcher)
  form      device | host (staging copies) | async (sync=False) | reuse (a second call on the same cache with other operands)
  families  tridiag, tridiag_nl; lap5, lap5_nl on even nx (a lazy launcher; nx = 2: every pair touches both edges) and lap5 on odd nx
            (none: the cache falls back); sparse on the wide / tall / ragged / tiny patterns of tests/exact_general.py and three small
            rectangular ones (M = 1, odd M)
  operands  OPERANDS below.  The families tagged all_nan (NaN in x, Inf in v, a dot that overflows, eps = 0) make EVERY value NaN; they
            run on tridiag_nl only (a row without entries of a sparse pattern would stay 0 / Inf = 0), one case per route and element
            type.  Every other case keeps at least exact_general.MIN_FINITE of its values finite and has a finite, non-zero eps."""
import functools

import numpy as np

import color_model
import exact_general as G
import exact_model as X
import jvp_model as J
from exact_operands import operands as _operands

MIN_FINITE = G.MIN_FINITE
SIZES = (1, 2, 3, 63, 64, 65, 257, 1023, 1025, 16383, 16384, 16385, 16386, 40001, 600001)
SMALL_OFF_SIZES = (1, 2, 3, 65, 257, 1025)
SEARCH_CUS = 256                       # the CU count the seed search assumes (an MI355X); the GPU test models the device's own
OPERANDS = ("generic", "dot_neg", "x_zero", "unit_v", "abs_above", "abs_below", "relstep", "signed_zeros", "huge_x", "sub_ev",
            "nan_x", "inf_v", "overflow", "eps0")
ALL_NAN = ("nan_x", "inf_v", "overflow", "eps0")


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(M, N, colptr, rowval), 1-based int64: exact_general's, or rect_<M>x<N>."""
    if name.startswith("rect_"):
        M, N = (int(s) for s in name[5:].split("x"))
        return (M, N) + color_model.random_band(M, N, 3, max(2, M // 8), M + 3 * N)
    return G.pattern(name)


def shape(case):
    fam, prm = case["family"], case["prm"]
    if fam == "sparse":
        return pattern(prm[0])[:2]
    n = prm[0] if fam.startswith("tridiag") else prm[0] * prm[1]
    return n, n


def np_dtype(case):
    return np.float64 if case["dtype"] == "f64" else np.float32


def has_lazy(case):
    """The built-in family has a lazy JVP launcher (csrc/fdjac_f_jvp.hip, has_lazy_jvp)."""
    fam = case["family"]
    return fam.startswith("tridiag") or (fam.startswith("lap5") and case["prm"][0] % 2 == 0)


def route(case):
    N = shape(case)[1]
    if N <= J.SMALL_N and not case["small_off"]:
        return "small"
    if case["declined"]:
        return "declined"
    if case["lazy"] and has_lazy(case):
        fin = case["f_in"] and case["fdtype"] == "forward"
        return "lazy_quotient" if case["quotient"] and not fin and not case["outoff"] else "lazy_values"
    return "mat_scalar" if case["xoff"] else "mat_paired"


def dot_order(case):
    r = route(case)
    return "small" if r == "small" else ("scalar" if case["xoff"] else "paired")


def counts(case):
    """(launches of f!, points evaluated) the route must report."""
    r, central = route(case), case["fdtype"] == "central"
    fin = case["f_in"] and not central
    points = 2 if central or not fin else 1
    if r in ("small", "lazy_values", "lazy_quotient"):
        return 1, points
    return (2 if not central and not fin else 1), points


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def operands(fam, N, dtype, seed):
    """(x, v, relstep, absstep)."""
    rng = np.random.default_rng(seed)
    f32 = np.dtype(dtype) == np.dtype(np.float32)
    x = rng.random(N) - 0.25
    v = rng.random(N) - 0.5
    rel = ab = None
    if fam == "dot_neg":
        v = -(0.25 + rng.random(N)) * x
    elif fam in ("x_zero", "eps0"):
        x = np.zeros(N)
        if fam == "eps0":
            ab = 0.0
    elif fam == "unit_v":
        v = np.zeros(N)
        x[N // 3] = 0.0
        v[N // 3] = 1.0
    elif fam == "abs_above":
        ab = 0.25
    elif fam == "abs_below":
        v = (0.25 + rng.random(N)) * x
        ab = 1e-12
    elif fam == "relstep":
        rel = 3e-5
    elif fam == "signed_zeros":
        x = _operands("signed_zeros", N, 1, np.float64, seed)[0]
        v[rng.random(N) < 0.3] = -0.0
        v[rng.random(N) < 0.2] = 0.0
    elif fam == "huge_x":            # x + eps v == x: every numerator is +0, the quotient a zero with eps's sign
        x = 2.0 ** (30 if f32 else 100) * (1 + rng.random(N)) * np.where(rng.random(N) < 0.5, -1, 1)
        v = (1e-20 if f32 else 1e-30) * (rng.random(N) - 0.5)
    elif fam == "sub_ev":            # x and eps v subnormal (the dot underflows: eps = absstep)
        unit, kx, kv = (2.0 ** -149, 1000, 10 ** 5) if f32 else (5e-324, 10 ** 6, 10 ** 12)
        x = unit * rng.integers(-kx, kx, N).astype(np.float64)
        v = unit * rng.integers(-kv, kv, N).astype(np.float64)
    elif fam == "nan_x":
        x[N // 2] = np.nan
    elif fam == "inf_v":
        v[N // 2] = np.inf
    elif fam == "overflow":
        x = (3e38 if f32 else 1e200) * np.ones(N)
        v = x * (1 - 0.01 * rng.random(N))
    elif fam != "generic":
        raise ValueError(fam)
    return x.astype(dtype), v.astype(dtype), rel, ab


@functools.lru_cache(maxsize=None)
def _searched_seed(N, seed):
    """Float64 generic operands: the first of 40 seeds at which the three summation orders give the most different step sizes (three,
    where the orders differ at all at this N)."""
    best, best_n = seed, 0
    for s in range(seed, seed + 40):
        x, v, _r, _a = operands("generic", N, np.float64, s)
        n = len({float(J.epsilon(J.dot(x, v, o, SEARCH_CUS), "forward")) for o in ("small", "scalar", "paired")})
        if n > best_n:
            best, best_n = s, n
        if n == 3:
            break
    return best


# ---- the table of cases --------------------------------------------------------------------------------------------------------------
def _case(family, prm, dtype="f64", fdtype="forward", ops="generic", lazy=True, quotient=True, xoff=0, outoff=0, form="device",
          declined=False, small_off=False, f_in=False, dir=1.0):
    c = dict(family=family, prm=tuple(prm), dtype=dtype, fdtype=fdtype, ops=ops, lazy=lazy, quotient=quotient, xoff=xoff, outoff=outoff,
             form=form, declined=declined, small_off=small_off, f_in=f_in, dir=dir)
    c["all_nan"] = ops in ALL_NAN
    c["id"] = "-".join([family, "x".join(str(p) for p in prm), dtype, fdtype + ("m" if dir < 0 else ""), route(c)] +
                       [t for t, on in (("nolazy", not lazy and has_lazy(c)), ("noq", lazy and not quotient and has_lazy(c)),
                                        ("xoff", xoff), ("outoff", outoff), (form, form != "device"), ("small0", small_off),
                                        ("fin", f_in), (ops, ops != "generic")) if on])
    return c


# (lazy, quotient, xoff, outoff): the ways a cache and its arrays can be set up
_DEFAULT, _VALUES, _MAT, _MAT_X, _LAZY_X, _LAZY_OUT, _MAT_OUT = ((True, True, 0, 0), (True, False, 0, 0), (False, False, 0, 0),
                                                                 (False, False, 1, 0), (True, True, 1, 0), (True, True, 0, 1),
                                                                 (False, False, 0, 1))


def _setup(s):
    return dict(lazy=s[0], quotient=s[1], xoff=s[2], outoff=s[3])


def _build_cases():
    out = []
    fd2 = ("forward", "central")
    # A. the sizes with the library's own routing (small up to 16384, the family's lazy launcher above), and the materialised forms above it
    for i, n in enumerate(SIZES):
        fam, fdt = ("tridiag", "tridiag_nl")[i % 2], fd2[(i // 2) % 2]
        out.append(_case(fam, (n,), fdtype=fdt))
        if n > J.SMALL_N:
            out += [_case(fam, (n,), fdtype=fdt, **_setup(s)) for s in (_VALUES, _MAT, _MAT_X)]
        if n in (1, 3, 65, 1025, 16384, 16385, 40001, 600001):
            out.append(_case(fam, (n,), "f32", fd2[1 - (i // 2) % 2]))
            if n > J.SMALL_N:
                out += [_case(fam, (n,), "f32", fd2[1 - (i // 2) % 2], **_setup(s)) for s in (_MAT, _MAT_X)]
    # B. the large kernels at tiny N (FDJAC_SMALL=0): n2 == 0, tail only, one partial
    for i, n in enumerate(SMALL_OFF_SIZES):
        for k, s in enumerate((_MAT, _MAT_X, _DEFAULT, (True, False, 1, 0))):
            out.append(_case(("tridiag", "tridiag_nl")[k % 2], (n,), fdtype=fd2[(i + k) % 2], small_off=True, **_setup(s)))
            if n in (1, 2, 3, 257):
                out.append(_case(("tridiag_nl", "tridiag")[k % 2], (n,), "f32", fd2[(i + k + 1) % 2], small_off=True, **_setup(s)))
    for n in (3, 1025):
        for s in (_MAT, _DEFAULT):
            out += [_case("tridiag_nl", (n,), dt, small_off=True, f_in=True, **_setup(s)) for dt in ("f64", "f32")]
    # C. every family on every route
    for fam in ("tridiag", "tridiag_nl"):
        for dt in ("f64", "f32"):
            for fdt in fd2:
                out += [_case(fam, (40001,), dt, fdt, **_setup(s)) for s in (_LAZY_X, _LAZY_OUT, _MAT_OUT)]
                out.append(_case(fam, (40001,), dt, fdt, form="host"))
            out += [_case(fam, (40001,), dt, "forward", f_in=True, **_setup(s)) for s in (_DEFAULT, _MAT, _MAT_X)]
            out += [_case(fam, (40001,), dt, "forward", f_in=True, form="host"), _case(fam, (1025,), dt, "forward", f_in=True),
                    _case(fam, (1025,), dt, "central", f_in=True), _case(fam, (1025,), dt, "forward", form="host"),
                    _case(fam, (1025,), dt, "central", **_setup(_MAT_OUT)), _case(fam, (1025,), dt, "forward", **_setup(_LAZY_X))]
    for fam in ("lap5", "lap5_nl"):
        for dt in ("f64", "f32"):
            for g, grid in enumerate(((2, 1), (2, 3), (4, 5))):
                out.append(_case(fam, grid, dt, fd2[g % 2]))
                for k, s in enumerate((_DEFAULT, _VALUES, _MAT, _MAT_X, _LAZY_OUT)):
                    out.append(_case(fam, grid, dt, fd2[(g + k + 1) % 2], small_off=True, **_setup(s)))
                out.append(_case(fam, grid, dt, "forward", small_off=True, f_in=True))
            for k, s in enumerate((_DEFAULT, _VALUES, _MAT, _MAT_X, _LAZY_OUT, _LAZY_X)):
                out.append(_case(fam, (130, 131), dt, fd2[k % 2], **_setup(s)))
            out += [_case(fam, (130, 131), dt, "central", form="host"), _case(fam, (130, 131), dt, "forward", f_in=True)]
    for dt in ("f64", "f32"):           # no lazy launcher on an odd nx: the cache falls back to the materialised points
        out += [_case("lap5", (7, 9), dt, "forward"), _case("lap5", (7, 9), dt, "central", small_off=True),
                _case("lap5", (7, 9), dt, "forward", small_off=True, xoff=1), _case("lap5", (131, 131), dt, "forward"),
                _case("lap5", (131, 131), dt, "central", xoff=1), _case("lap5", (131, 131), dt, "forward", f_in=True, outoff=1)]
    for p in ("wide", "tall", "ragged", "tiny_1", "tiny_2", "tiny_3", "tiny_65", "tiny_257", "rect_1x37", "rect_301x77", "rect_77x301"):
        out += [_case("sparse", (p,), "f64", "forward"), _case("sparse", (p,), "f64", "central", f_in=True),
                _case("sparse", (p,), "f64", "forward", small_off=True, f_in=True), _case("sparse", (p,), "f64", "central", small_off=True, xoff=1),
                _case("sparse", (p,), "f32", "central"), _case("sparse", (p,), "f32", "forward", small_off=True, xoff=1)]
        if p in ("wide", "tall", "rect_1x37", "rect_301x77"):
            out += [_case("sparse", (p,), dt, fdt, small_off=so, **kw) for dt in ("f64", "f32") for fdt, so, kw in
                    (("forward", False, dict(form="host", f_in=True)), ("central", True, dict(form="host")),
                     ("forward", True, dict(outoff=1)), ("central", False, dict(outoff=1, xoff=1)), ("central", True, dict()))]
    # D. the operand families, on five set-ups; dir = -1
    bases = (dict(family="tridiag_nl", prm=(1025,)), dict(family="tridiag_nl", prm=(1025,), small_off=True),
             dict(family="tridiag_nl", prm=(1025,), small_off=True, lazy=False, xoff=1), dict(family="sparse", prm=("wide",), small_off=True),
             dict(family="lap5_nl", prm=(4, 5), small_off=True, quotient=False))
    k = 0
    for ops in OPERANDS[1:]:
        if ops in ALL_NAN:
            continue
        for dt in ("f64", "f32"):
            for b in bases:
                out.append(_case(dtype=dt, fdtype=fd2[k % 2], ops=ops, **b))
                k += 1
    for dt in ("f64", "f32"):
        for fdt in fd2:
            out += [_case(dtype=dt, fdtype=fdt, dir=-1.0, **b) for b in bases[:4]]
        # (x + eps v == x: the numerator is +0 and the quotient's sign is eps's -- in the central rule dir must NOT reach it)
        out += [_case(dtype=dt, fdtype=fdt, dir=-1.0, ops="huge_x", **b) for fdt in fd2 for b in bases[:2]]
    # (all_nan: each family once per element type, each route and element type at most once)
    nan_bases = (bases[0], bases[1], bases[2], dict(family="tridiag_nl", prm=(1025,), small_off=True, lazy=False),
                 dict(family="tridiag_nl", prm=(1025,), small_off=True, quotient=False))
    for i, ops in enumerate(ALL_NAN):
        out += [_case(dtype="f64", fdtype=fd2[i % 2], ops=ops, **nan_bases[i]),
                _case(dtype="f32", fdtype=fd2[1 - i % 2], ops=ops, **nan_bases[(i + 1) % 5])]
    # E. a launcher that declines; fd_jvp_async; a second call on the same cache
    out += [_case("tridiag_nl", (40001,), "f64", "forward", declined=True), _case("tridiag_nl", (40001,), "f32", "central", declined=True),
            _case("tridiag", (40001,), "f64", "central", declined=True, xoff=1), _case("tridiag", (40001,), "f32", "forward", declined=True, f_in=True),
            _case("lap5", (130, 131), "f32", "forward", declined=True, quotient=False), _case("lap5_nl", (130, 131), "f64", "central", declined=True),
            _case("tridiag", (3,), "f64", "forward", declined=True, small_off=True), _case("tridiag_nl", (65,), "f64", "central", declined=True, small_off=True),
            _case("sparse", ("rect_301x77",), "f64", "forward", declined=True, small_off=True),
            _case("tridiag_nl", (40001,), "f64", "forward", declined=True, outoff=1)]
    for dt in ("f64", "f32"):
        out += [_case("tridiag_nl", (40001,), dt, "forward", form="async"), _case("tridiag_nl", (1025,), dt, "central", form="async"),
                _case("lap5", (131, 131), dt, "forward", form="async"), _case("lap5_nl", (130, 131), dt, "central", form="async", quotient=False)]
        out += [_case("tridiag", (1025,), dt, "forward", form="reuse"), _case("tridiag", (40001,), dt, "central", form="reuse", lazy=False),
                _case("tridiag", (40001,), dt, "forward", form="reuse", lazy=False, xoff=1), _case("lap5_nl", (130, 131), dt, "forward", form="reuse"),
                _case("lap5_nl", (130, 131), dt, "central", form="reuse", quotient=False),
                _case("sparse", ("rect_77x301",), dt, "forward", form="reuse", small_off=True)]
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _build_cases()


def inputs(case, call=0):
    """Everything a run of the case needs on the host: M, N, x, v, f_in, rel, ab, dir, dtype, f (the model's residual).  call = 1: the
    operands of a `reuse` case's second call."""
    M, N = shape(case)
    dtype = np_dtype(case)
    seed = 31 * N + M + 7 * OPERANDS.index(case["ops"]) + 100003 * call
    if case["ops"] == "generic" and N >= 65:
        seed = _searched_seed(N, seed)
    x, v, rel, ab = operands(case["ops"], N, dtype, seed)
    f_in = (np.random.default_rng(seed + 1).random(M) - 0.5).astype(dtype) if case["f_in"] else None     # any values: subtracted as given
    if case["family"] == "sparse":
        f = X.fixture("sparse", *pattern(case["prm"][0]))
    else:
        f = X.fixture(case["family"], *case["prm"])
    return dict(M=M, N=N, x=x, v=v, f_in=f_in, rel=rel, ab=ab, dir=case["dir"], dtype=dtype, f=f)


def model(case, num_cus=SEARCH_CUS, call=0, order=None, epsilon=J.epsilon, jvp=J.jvp):
    """The model's own answer: (the M values, eps, the Float64 dot product) with the summation order of the case's route."""
    inp = inputs(case, call)
    t = J.dot(inp["x"], inp["v"], order or dot_order(case), num_cus)
    eps = epsilon(t, case["fdtype"], inp["rel"], inp["ab"], inp["dir"], inp["dtype"])
    return jvp(inp["f"], inp["x"], inp["v"], eps, case["fdtype"], inp["f_in"]), eps, t
