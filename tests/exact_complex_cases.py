"""The cases of tests/test_gpu_exact_complex.py: the COMPLEX STEP J[:, j] = imag(f(x + i eps mask_c)) / eps, eps = eps(T) (src/jacobians.jl:
623-648), on every Jacobian route of the rational built-in families against the pair model of tests/exact_model.py (fixture_complex,
colour_values_complex), bit for bit.  Pure numpy (the stencil patterns come from finitediff_jl_amd.patterns, itself pure numpy: neither
libfdjac nor torch is loaded) -- patterns, colourings, operands, the table of cases and the model's answer -- so that the CPU suite (tests/test_exact_complex_cpu.py) evaluates every GPU case with the model alone.  Test infrastructure only.

  routes     handover   k_perturb MODE 2 -> the complex f! -> the imag-only decompression (FDJAC_LAZY_STORE=0, no lazy launcher): all six
                        families; `dest` = csc_list / csc_window (FDJAC_WINDOW 0 / 1), banded, tridiagonal, dense (a dense J with a CSC
                        sparsity), colwindow (a column window), colorrange (two colour-owning plans)
             lazy       set_lazy(f, imag_only=True / False): the tridiagonal and 5-point lazy-point launchers (imaginary parts as a real
                        array / (re, im) pairs), decompressed by the library
             cols       the column store of the built-in sparse residual and of the 7-point family (k_csc_store_cols_cplx)
             jit        a runtime-compiled row functor, generic in the point's value type (fd_csc_store_cols_cplx)
             terms      a runtime-compiled separable-terms functor (SPARSE_TERMS of tests/test_gpu_jit.py)
             dense      the dense uncoloured arm: N <= 64, every column its own colour, a dense J
  colourings cycC_S     (j + S) mod C + 1 (cyclic); noncyc: cyc3_0 with every 30th column moved to a fourth colour (valid, not cyclic);
                        none: the same with columns 0-coloured; ones: every column colour 1 (INVALID wherever two columns share a row:
                        the colour's point is the promise, not the column's); own: column j has colour j + 1 (more than 253 colours
                        on random_band600: the Int32 colour width); the named colourings of tests/exact_store_cases.py otherwise
  operands   FAMILIES64 / FAMILIES32.  The step is eps(T) whatever x is, so the families that move the step size of a forward
             difference (eps_2p100_*, num_2p800, cancel ...) have nothing to say here.  `re_overflow` scales x so that the REAL part of
             the nonlinear term overflows in most rows while every imaginary part and its quotient by eps stay finite: cubic families
             (x x) x+ at |x| ~ 1e150 (Float32: 3e14), the quadratic sparse term (q x) x at 1e160 (Float32: 3e20).  `f32_im_subnormal`:
             |x| ~ 2^-104, so that every product x 2^-23 in an imaginary part is a Float32 subnormal.  On these residuals such a product
             is always ADDED to a multiple of eps next and absorbed there (no stored bit can depend on it: eps^3 is still a normal
             number, so no final imaginary part is subnormal); the family pins that nothing else happens to such rows -- a flush that
             turned the sum itself into 0 or a NaN would show."""
import functools

import numpy as np

import exact_general as G
import exact_model as X
import exact_store_cases as S
from finitediff_jl_amd import patterns as P

MIN_FINITE = G.MIN_FINITE
FAMILIES64 = ["ordinary", "signed_zeros", "nan_inf", "tiny_1e-200", "subnormal", "re_overflow"]
FAMILIES32 = ["ordinary", "signed_zeros", "f32_subnormal", "nan_inf", "re_overflow", "f32_im_subnormal"]
TRIDIAG_SIZES = [1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025]
TRIDIAG_OPERAND_N = 70_001
LAP5_GRIDS = [(nx, ny) for nx in (6, 254, 256, 258) for ny in (2, 3, 5)]
LAP5_OPERAND_GRID = (258, 40)
COL_WINDOW = (1235, 5000)           # (random_band: an odd first column)
COLOR_RANGES = ((0, 2), (2, None))
ROUTES = ("handover", "lazy", "cols", "jit", "terms", "dense")


def np_dtype(case):
    return np.float64 if case["dtype"] == "f64" else np.float32


@functools.lru_cache(maxsize=None)
def pattern(fixture, shape):
    """(M, N, colptr, rowval), 1-based int64; shape: (N,), (nx, ny), a 7-point name of exact_store_cases.LAP7, or a pattern's name."""
    if fixture in ("tridiag", "tridiag_nl"):
        N = shape[0]
        cp, rv = P.tridiag_csc(N)
        return N, N, np.asarray(cp, np.int64), np.asarray(rv, np.int64)
    if fixture in ("lap5", "lap5_nl"):
        nx, ny = shape
        cp, rv = P.lap5_csc(nx, ny)
        return nx * ny, nx * ny, np.asarray(cp, np.int64), np.asarray(rv, np.int64)
    if shape[0].startswith("full_"):                # the dense uncoloured arm: every entry of an n x n matrix
        n = int(shape[0][5:])
        return n, n, np.arange(n + 1, dtype=np.int64) * n + 1, np.tile(np.arange(1, n + 1, dtype=np.int64), n)
    return S.pattern(shape[0])


@functools.lru_cache(maxsize=None)
def colouring(fixture, shape, kind):
    """The colour vector (int64, 1-based, 0 = no colour)."""
    M, N, colptr, rowval = pattern(fixture, shape)
    j = np.arange(N, dtype=np.int64)
    if kind == "ones":
        return np.ones(N, np.int64)
    if kind == "own":
        return j + 1
    if kind.startswith("cyc"):
        C, shift = (int(v) for v in kind[3:].split("_"))
        return (j + shift) % C + 1
    if kind in ("noncyc", "none"):
        g = j % 3 + 1
        g[7::30] = 4
        if kind == "none":
            g[np.unique([N // 7, N // 3, N // 2, (2 * N) // 3, N - 1])] = 0
        return g
    if fixture in ("lap5", "lap5_nl"):
        g = np.asarray(P.lap5_colors(*shape), np.int64).copy()
        if kind == "stencil_none5":
            g[np.unique([N // 7, N // 3, N // 2, (2 * N) // 3, N - 1])] = 0
        else:
            assert kind == "stencil", kind
        return g
    return S.colouring(shape[0], kind)


def _re_overflow_scale(fixture, dtype):
    if fixture == "sparse":
        return 1e160 if dtype == np.float64 else 3e20
    return 1e150 if dtype == np.float64 else 3e14


def operands(case, N, colors):
    """x in the case's element type (relstep and absstep do not enter the complex step)."""
    dtype = np_dtype(case)
    C = int(colors.max())
    seed = 7 * N + C
    fam = case["family"]
    if fam == "re_overflow":
        rng = np.random.default_rng(seed)
        return ((rng.random(N) - 0.25) * _re_overflow_scale(case["fixture"], dtype)).astype(dtype)
    if fam == "f32_im_subnormal":
        rng = np.random.default_rng(seed)
        return ((rng.random(N) - 0.25) * 2.0 ** -104).astype(dtype)
    return G.operands(fam, None, colors, dtype, seed, N=N)[0]


# ---- the table of cases --------------------------------------------------------------------------------------------------------------
def _shape_name(shape):
    return "x".join(str(s) for s in shape)


def _case(route, fixture, shape, col, dtype="f64", family="ordinary", dest="csc_list", imag_only=None):
    shape = tuple(shape) if not isinstance(shape, str) else (shape,)
    cid = "-".join([route, fixture, _shape_name(shape), col, dtype, family, dest] +
                   ([] if imag_only is None else ["imag" if imag_only else "pairs"]))
    return dict(id=cid, route=route, fixture=fixture, shape=shape, colouring=col, dtype=dtype, family=family, dest=dest, imag_only=imag_only)


def _build_cases():
    out = []
    both = ("f64", "f32")
    # ---- the hand-over path
    tri_dest = ("csc_list", "csc_window", "banded", "tridiagonal")
    for i, N in enumerate(TRIDIAG_SIZES):
        for k, dt in enumerate(both):
            col = "own" if N < 3 else ("cyc3_0", "cyc4_1", "cyc5_2", "noncyc")[(i + k) % 4]
            out.append(_case("handover", ("tridiag", "tridiag_nl")[(i + k) % 2], (N,), col, dt, dest=tri_dest[(i + 2 * k) % 4]))
    for i, fam in enumerate(FAMILIES64):
        for fixture in ("tridiag", "tridiag_nl"):
            out.append(_case("handover", fixture, (TRIDIAG_OPERAND_N,), "cyc3_1", family=fam, dest=tri_dest[(i + (fixture == "tridiag")) % 4]))
    for i, fam in enumerate(FAMILIES32):
        out.append(_case("handover", "tridiag_nl", (TRIDIAG_OPERAND_N,), "cyc3_1", "f32", fam, dest=tri_dest[i % 4]))
    for dest in tri_dest:
        out += [_case("handover", "tridiag_nl", (513,), "none", dest=dest), _case("handover", "tridiag_nl", (513,), "ones", dest=dest)]
    out += [_case("handover", "tridiag_nl", (1025,), "ones", "f32", "f32_im_subnormal"),
            _case("handover", "tridiag", (1025,), "ones", "f64", "nan_inf"), _case("handover", "tridiag_nl", (1025,), "ones", "f64", "signed_zeros")]
    for i, (nx, ny) in enumerate(LAP5_GRIDS):
        for k, dt in enumerate(both):
            out.append(_case("handover", ("lap5", "lap5_nl")[(i + k) % 2], (nx, ny), "stencil", dt, dest=("csc_list", "csc_window")[(i + k) % 2]))
    for fam in FAMILIES64:
        out.append(_case("handover", "lap5_nl", LAP5_OPERAND_GRID, "stencil", family=fam, dest="csc_window"))
    for fam in FAMILIES32:
        out.append(_case("handover", "lap5_nl", LAP5_OPERAND_GRID, "stencil", "f32", fam))
    out += [_case("handover", "lap5_nl", (70, 40), "stencil_none5"), _case("handover", "lap5_nl", (70, 40), "ones", dest="csc_window"),
            _case("handover", "lap5", (70, 40), "ones", "f32", "f32_im_subnormal"), _case("handover", "lap5_nl", (70, 40), "ones", "f32", "f32_im_subnormal"), _case("handover", "lap5", (70, 40), "stencil", dest="dense")]
    for name in S.LAP7:
        out += [_case("handover", "lap7", name, "greedy"), _case("handover", "lap7", name, "ones", "f32")]
    for fam in FAMILIES64:
        out.append(_case("handover", "lap7", "lap7_33x4x9", "small" if fam == "nan_inf" else "greedy", family=fam))
    for fam in FAMILIES32:
        out.append(_case("handover", "lap7", "lap7_33x4x9", "small" if fam == "nan_inf" else "greedy", "f32", fam))
    out.append(_case("handover", "lap7", "lap7_33x4x9", "none5", dest="dense"))
    for fam in FAMILIES64:
        out += [_case("handover", "sparse", "random_band", "greedy", family=fam), _case("handover", "sparse", "random_band", "invalid6", family=fam, dest="csc_window")]
    for fam in FAMILIES32:
        out.append(_case("handover", "sparse", "random_band", "invalid6", "f32", fam))
    for pat in ("wide", "tall", "ragged400", "tiny_1", "tiny_2", "tiny_3"):
        out += [_case("handover", "sparse", pat, "greedy"), _case("handover", "sparse", pat, "ones", "f32")]
    out += [_case("handover", "sparse", "random_band", "none5"), _case("handover", "sparse", "random_band600", "greedy", dest="dense"),
            _case("handover", "sparse", "random_band600", "invalid6", dest="dense"), _case("handover", "sparse", "wide", "none5", dest="dense"),
            _case("handover", "sparse", "random_band600", "own"),
            _case("handover", "sparse", "random_band", "greedy", dest="colwindow"), _case("handover", "sparse", "random_band", "invalid6", dest="colwindow"),
            _case("handover", "sparse", "random_band", "greedy", dest="colorrange"), _case("handover", "sparse", "random_band", "invalid6", "f32", dest="colorrange")]
    # ---- the lazy-point launchers: imaginary parts only, and (re, im) pairs
    for i, N in enumerate(TRIDIAG_SIZES):
        if N < 3:
            continue                  # (the family has no lazy launcher below three columns)
        for k, dt in enumerate(both):
            out.append(_case("lazy", ("tridiag_nl", "tridiag")[(i + k) % 2], (N,), ("cyc3_0", "cyc4_1", "noncyc", "ones")[(i + k) % 4] if N > 3 else "cyc3_0",
                             dt, imag_only=bool((i + k) % 2)))
    for fam in FAMILIES64:
        out += [_case("lazy", "tridiag_nl", (TRIDIAG_OPERAND_N,), "cyc3_1", family=fam, imag_only=True),
                _case("lazy", "tridiag_nl", (TRIDIAG_OPERAND_N,), "cyc3_1", family=fam, imag_only=False)]
    for i, fam in enumerate(FAMILIES32):
        out.append(_case("lazy", "tridiag_nl", (TRIDIAG_OPERAND_N,), "cyc3_1", "f32", fam, imag_only=bool(i % 2)))
    for i, (nx, ny) in enumerate(LAP5_GRIDS):
        for k, dt in enumerate(both):
            out.append(_case("lazy", ("lap5_nl", "lap5")[(i + k) % 2], (nx, ny), "stencil", dt, imag_only=bool((i + k) % 2)))
    for i, fam in enumerate(FAMILIES64):
        out.append(_case("lazy", "lap5_nl", LAP5_OPERAND_GRID, "stencil", family=fam, imag_only=bool(i % 2)))
    for i, fam in enumerate(FAMILIES32):
        out.append(_case("lazy", "lap5_nl", LAP5_OPERAND_GRID, "stencil", "f32", fam, imag_only=not bool(i % 2)))
    out += [_case("lazy", "lap5_nl", (70, 40), "ones", imag_only=True), _case("lazy", "lap5_nl", (70, 40), "stencil_none5", imag_only=False)]
    # ---- the column stores
    for fam in FAMILIES64:
        out += [_case("cols", "sparse", "random_band", "greedy", family=fam), _case("cols", "sparse", "random_band", "invalid6", family=fam),
                _case("cols", "lap7", "lap7_33x4x9", "small" if fam == "nan_inf" else "greedy", family=fam),
                _case("jit", "sparse", "random_band", "greedy", family=fam), _case("terms", "sparse", "random_band", "greedy", family=fam)]
    for fam in FAMILIES32:
        out += [_case("jit", "sparse", "random_band", "invalid6" if fam == "signed_zeros" else "greedy", "f32", fam),
                _case("terms", "sparse", "random_band", "greedy", "f32", fam),
                _case("cols", "sparse", "random_band", "invalid6" if fam != "ordinary" else "greedy", "f32", fam),
                _case("cols", "lap7", "lap7_33x4x9", "small" if fam == "nan_inf" else "greedy", "f32", fam)]
    for pat in ("wide", "tall", "ragged400", "tiny_1", "tiny_2", "tiny_3"):
        out += [_case("cols", "sparse", pat, "greedy"), _case("cols", "sparse", pat, "ones", "f32"), _case("jit", "sparse", pat, "greedy")]
    out += [_case("cols", "sparse", "random_band", "none5"), _case("cols", "sparse", "random_band", "many"),
            _case("cols", "sparse", "random_band600", "own"), _case("cols", "sparse", "random_band", "greedy", dest="colwindow"),
            _case("cols", "sparse", "random_band", "invalid6", dest="colorrange"),
            _case("jit", "sparse", "random_band", "invalid6"), _case("jit", "sparse", "random_band", "none5"),
            _case("jit", "sparse", "random_band600", "own"), _case("jit", "sparse", "ragged400", "ones"),
            _case("jit", "sparse", "random_band", "greedy", "f32"), _case("jit", "sparse", "random_band", "invalid6", "f32", "signed_zeros"),
            _case("terms", "sparse", "random_band", "none5"), _case("terms", "sparse", "ragged400", "greedy"), _case("terms", "sparse", "tiny_2", "greedy")]
    for name in S.LAP7:
        out += [_case("cols", "lap7", name, "greedy"), _case("cols", "lap7", name, "ones"), _case("cols", "lap7", name, "none5", "f32")]
    # ---- the dense uncoloured arm
    for n in (1, 2, 7, 64):
        for dt in both:
            out.append(_case("dense", "sparse", "full_%d" % n, "own", dt, dest="dense"))
    out += [_case("dense", "sparse", "full_64", "own", family=fam, dest="dense") for fam in ("signed_zeros", "nan_inf", "re_overflow")]
    seen, uniq = set(), []          # (the per-shape and the per-family loops name a few cases twice: each stands once)
    for c in out:
        if c["id"] not in seen:
            seen.add(c["id"])
            uniq.append(c)
    return uniq


CASES = _build_cases()


def fixture_params(case):
    M, N, colptr, rowval = pattern(case["fixture"], case["shape"])
    fx = case["fixture"]
    if fx == "sparse":
        return (M, N, colptr, rowval)
    if fx == "lap7":
        return S.LAP7[case["shape"][0]]
    return case["shape"]


def inputs(case, smul=X.c_smul):
    """Everything a run of the case needs on the host: M, N, colptr, rowval, colors, c0, C, x, dtype, f (the pair model's residual)."""
    M, N, colptr, rowval = pattern(case["fixture"], case["shape"])
    colors = colouring(case["fixture"], case["shape"], case["colouring"])
    C = int(colors.max())
    x = operands(case, N, colors)
    f = X.fixture_complex(case["fixture"], *fixture_params(case), smul=smul)
    return dict(M=M, N=N, colptr=colptr, rowval=rowval, colors=colors, c0=colors - 1, C=C, x=x, dtype=np_dtype(case), f=f)


def layout(case, inp, part=None):
    """D -> [the arrays the case's destination holds]; part = (c_lo, c_hi): a colour-owning plan's share (zeros elsewhere)."""
    cp, rv, c0, M, N = inp["colptr"], inp["rowval"], inp["c0"], inp["M"], inp["N"]
    dest = case["dest"]
    if dest == "banded":
        return lambda D: [X.to_banded(D, c0, M, N, 1, 1)]
    if dest == "tridiagonal":
        return lambda D: list(X.to_tridiagonal(D, c0, N))
    if dest == "dense":
        return lambda D: [X.to_dense(D, c0, cp, rv, M, N)]
    if dest == "colwindow":
        a, b = COL_WINDOW
        return lambda D: [X.to_csc(D, c0, cp, rv)[cp[a] - 1:cp[b] - 1]]
    if part is not None:
        own = np.where((c0 >= part[0]) & (c0 < part[1]), c0, -1)
        return lambda D: [X.to_csc(D, own, cp, rv)]
    return lambda D: [X.to_csc(D, c0, cp, rv)]


def parts(case, C):
    return [None] if case["dest"] != "colorrange" else [(a, C if b is None else b) for a, b in COLOR_RANGES]


def model(case, smul=X.c_smul):
    """The model's own answer: (the destination's arrays, eps)."""
    inp = inputs(case, smul)
    eps = X.complex_epsilons(inp["C"], inp["dtype"])
    D = X.colour_values_complex(inp["f"], inp["x"], inp["c0"], inp["C"], eps)
    return layout(case, inp)(D), eps


def model_key(case):
    """Cases with equal keys have the same model answer (the route and the hand-over form do not enter it)."""
    dest = case["dest"] if case["dest"] in ("banded", "tridiagonal", "dense", "colwindow") else None
    return (case["fixture"], case["shape"], case["colouring"], case["dtype"], case["family"], dest)
