"""The cases of tests/test_gpu_exact_store.py: the STORING routes of general CSC patterns (fd_csc_store_cols, fd_csc_store_cols_win,
fd_csc_store_rows, fd_csc_store_ents, k_f_lap7_store_cols, a runtime-compiled row functor, a runtime-compiled separable-terms functor)
against the exact host model (tests/exact_model.py).  Pure numpy, built from the patterns of tests/exact_general.py and the operand
families of tests/exact_operands.py, so that the CPU suite (tests/test_exact_model.py) evaluates every case with the model alone.
Test infrastructure only.

  routes       cols        FD_F_SPARSE through the plain column kernel (an invalid colouring, M != N, or N <= 3)
               win         FD_F_SPARSE on a square, locally banded pattern with a verified colouring: the windowed column kernel for a
                           forward difference that forms f(x) itself; with a caller's f_in or a central difference the family takes a
                           column kernel of its own (entry-balanced) -- the case names the launch it must report (`launch`)
               rows, ents  FD_F_SPARSE on a plan that keeps its pattern by rows: the row-wise store / its entry-parallel form
               lap7        the 7-point family: its column kernel (a verified colouring), else the plain column kernel
               jit         a runtime-compiled row functor that restates SparseF::row from device pointers (windowed / plain)
               terms,      a runtime-compiled separable-terms functor with the same term: the row-wise store, entry-parallel with
               terms_ents  FDJAC_ROWS_ENTS=1
  patterns     random_band (6000 columns, 19 greedy colours: the medium pattern of every FD_F_SPARSE route), wide / tall (M < N, M > N),
               ragged400 (400 x 400: empty rows, every seventh column empty, one-entry rows, one dense row of 40 entries -- more than
               the 32 the model sums term by term and the 14 the row-wise store keeps in registers), rows12 (3000 columns, ~12.5 entries
               per row: a tile of 256 rows holds more than the 3072 entries the row-wise store stages, and more than the 2048 of the
               entry-parallel form, which such a plan does not build), tiny_1 / 2 / 3, lap7 grids 7 x 5 x 3, 1 x 1 x 40, 33 x 4 x 9 (medium)
  colourings   greedy (color_model.greedy, what matrix_colors gives; lap7: the grid's own seven), many (greedy spread over three times
               as many colours: still valid, more than kRegColors = 8), none5 (five columns without a colour), invalid6 (the folded
               colouring of tests/exact_general.py), ones (every column colour 1: the routes form the whole colour's point), small
               (7-point grids: the grid's seven classes hold 14 % of the columns each, so nan_inf gets an eighth class of 1 or 3
               columns to poison; N <= 3 cannot keep 90 % of 1 .. 4 stored values finite beside a NaN: no nan_inf there)
  operands     FAMILIES64 / FAMILIES32: the families of tests/test_gpu_exact_model.py that leave at least MIN_FINITE of the stored
               values finite.  phi is quadratic and the 7-point row cubic in x, so `huge_range` and `f32_huge` overflow every row and
               are left out, and `num_2p800` is RESIZED: |x_j| = 10^U(100, 150) with absstep 1e136 (7-point: 10^U(60, 100), 1e86) -- every
               value stays finite and the numerators reach from below 2^800 to above 2^900 (the absolute step is the step size).
               `num_2m900` is this table's own: the subnormal coordinates with the absolute step 1e-290 -- x + eps = eps, every numerator
               is about w eps, NON-ZERO and below 2^-900 (the three-argument rule's lower edge, which the zero numerators of
               eps_2m100_* cannot test: product and division both give 0 there), the quotients are of order 1.

div_sides() restates the two fall-back rules of fd_div_shared (include/fdjac_device.h) on the model's own numerators and divisors."""
import functools

import numpy as np

import color_model
import exact_general as G
import exact_model as X

MIN_FINITE = G.MIN_FINITE
FAMILIES64 = ["ordinary", "signed_zeros", "cancel", "eps_2p100_in", "eps_2p100_out", "eps_2m100_in", "eps_2m100_out", "num_2p800",
              "num_2m900", "tiny_1e-200", "subnormal", "nan_inf"]
FAMILIES32 = ["ordinary", "signed_zeros", "f32_subnormal", "nan_inf"]
EDGE_FAMILIES = ["ordinary", "signed_zeros", "nan_inf"]
DIV_FAMILIES = ["eps_2p100_in", "eps_2p100_out", "eps_2m100_in", "eps_2m100_out", "num_2p800", "num_2m900", "tiny_1e-200", "subnormal"]
LAP7 = {"lap7_7x5x3": (7, 5, 3), "lap7_1x1x40": (1, 1, 40), "lap7_33x4x9": (33, 4, 9)}
COL_WINDOW = (1235, 5000)          # (an odd first column; random_band)
COLOR_RANGES = ((0, 2), (2, None))  # colour ownership: two plans, each compared with the model's values of its colours, zeros elsewhere


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(M, N, colptr, rowval), 1-based int64."""
    if name == "rows12":
        return (3000, 3000) + color_model.random_band(3000, 3000, 14, 40, 8)
    if name == "ragged400":
        return G._ragged(400, 400, 200, 40, 12)
    if name in LAP7:
        nx, ny, nz = LAP7[name]
        N = nx * ny * nz
        k = np.arange(N, dtype=np.int64)
        i, j, l = k % nx, (k // nx) % ny, k // (nx * ny)
        has = np.stack([l > 0, j > 0, i > 0, np.ones(N, bool), i < nx - 1, j < ny - 1, l < nz - 1], axis=1)
        rows = np.stack([k - nx * ny, k - nx, k - 1, k, k + 1, k + nx, k + nx * ny], axis=1)
        colptr = np.concatenate([[0], np.cumsum(has.sum(axis=1))]).astype(np.int64) + 1
        return N, N, colptr, (rows[has] + 1).astype(np.int64)
    return G.pattern(name)


@functools.lru_cache(maxsize=None)
def colouring(pname, kind):
    """The colour vector (int64, 1-based, 0 = no colour)."""
    M, N, colptr, rowval = pattern(pname)
    if kind == "ones":
        return np.ones(N, np.int64)
    if kind == "invalid6":                  # (the folding of tests/exact_general.py: at most 6 colours, columns of one row in one colour)
        g = (colouring(pname, "greedy") - 1) % 5 + 1
        g[11::97] = 6
        _cp, _rows, row_ptr, row_cols = color_model._transpose(M, colptr, rowval, 1)
        r = int(np.nonzero(np.diff(row_ptr) >= 2)[0][0])
        g[row_cols[row_ptr[r] + 1]] = g[row_cols[row_ptr[r]]]
        return g
    if kind == "greedy":
        if pname in LAP7:
            nx, ny, _nz = LAP7[pname]
            k = np.arange(N, dtype=np.int64)
            return ((k % nx) + 2 * ((k // nx) % ny) + 3 * (k // (nx * ny))) % 7 + 1
        return color_model.greedy(M, N, colptr, rowval)
    g = colouring(pname, "greedy").copy()
    if kind == "many":
        return g + int(g.max()) * (np.arange(N) % 3)
    if kind == "small":                     # (7-point grids: one more, small colour class for nan_inf to poison -- columns far apart)
        g[[N // 2] if N < 1000 else [N // 5, N // 2, (4 * N) // 5]] = int(g.max()) + 1
        return g
    if kind == "none5":
        g[np.unique([N // 7, N // 3, N // 2, (2 * N) // 3, N - 1])] = 0
        return g
    raise ValueError(kind)


def operands(case, colors):
    """(x, relstep, absstep)."""
    N = pattern(case["pattern"])[1]
    dtype = np_dtype(case)
    seed = 7 * N + int(colors.max())
    if case["family"] == "num_2m900":
        x, _rel, _ab = G.operands("subnormal", case["pattern"], colors, dtype, seed, N=N)
        return x, 1e-300, 1e-290
    if case["family"] == "num_2p800":
        lo, hi, ab = (60, 100, 1e86) if case["fixture"] == "lap7" else (100, 150, 1e136)
        rng = np.random.default_rng(seed)
        x = 10.0 ** rng.uniform(lo, hi, N) * np.where(rng.random(N) < 0.5, -1, 1)
        return x.astype(dtype), 1e-300, ab
    return G.operands(case["family"], case["pattern"], colors, dtype, seed, N=N)


# ---- the table of cases --------------------------------------------------------------------------------------------------------------
def _case(pat, col, route, fdtype, dir=1.0, dtype="f64", family="ordinary", variant=None, launch=None):
    cid = "-".join([route, pat, col, fdtype + ("m" if dir < 0 else ""), dtype, family] + ([variant] if variant else []))
    fixture = "lap7" if route == "lap7" else "sparse"
    if launch is None:
        launch = {"cols": "cols", "win": "cols_win", "rows": "rows", "ents": "ents", "lap7": "family", "jit": "cols_win", "terms": "rows",
                  "terms_ents": "ents"}[route]
        if route == "win" and (fdtype == "central" or variant == "f_in"):
            launch = "family"
    return dict(id=cid, pattern=pat, colouring=col, route=route, fdtype=fdtype, dir=dir, dtype=dtype, family=family, variant=variant,
                fixture=fixture, launch=launch)


DIRS = (("forward", 1.0), ("forward", -1.0), ("central", 1.0))


def _build_cases():
    out = []
    # one medium pattern per route: the full Float64 operand matrix (forward and central; dir = -1 with ordinary, signed_zeros, nan_inf)
    medium = [("cols", "random_band", "invalid6"), ("win", "random_band", "greedy"), ("rows", "random_band", "greedy"),
              ("ents", "random_band", "greedy"), ("lap7", "lap7_33x4x9", "greedy"), ("jit", "random_band", "greedy"),
              ("terms", "random_band", "greedy"), ("terms_ents", "random_band", "greedy")]
    for route, pat, col in medium:
        for fam in FAMILIES64:
            for fdtype, dir in DIRS:
                if dir < 0 and fam not in EDGE_FAMILIES:
                    continue
                out.append(_case(pat, "small" if (route == "lap7" and fam == "nan_inf") else col, route, fdtype, dir=dir, family=fam))
        if route in ("jit", "terms", "terms_ents"):           # (one compiled module per functor: Float64)
            continue
        for fam in FAMILIES32:
            out.append(_case(pat, "small" if (route == "lap7" and fam == "nan_inf") else col, route, "central" if fam == "signed_zeros" else "forward",
                             dtype="f32", family=fam))
        out.append(_case(pat, col, route, "forward", dir=-1.0, dtype="f32", family="signed_zeros"))
    # call forms on the medium pattern: a caller's f_in, a column window, colour chunks, colour ownership
    for route, pat, col in medium:
        out.append(_case(pat, col, route, "forward", variant="f_in"))
        out.append(_case(pat, col, route, "forward", dir=-1.0, family="signed_zeros", variant="f_in"))
    for route, col, launch in (("cols", "invalid6", None), ("win", "greedy", None), ("jit", "greedy", None)):
        out += [_case("random_band", col, route, "forward", variant="colwindow", launch=launch),
                _case("random_band", col, route, "central", variant="colwindow", launch=launch)]
    # (a plan with a column window holds no row lists: the rows route is a whole-plan route)
    for route in ("cols", "win", "rows", "jit", "terms"):
        col = "invalid6" if route == "cols" else "greedy"
        out += [_case("random_band", col, route, "central", variant="chunked"), _case("random_band", col, route, "forward", variant="colorrange")]
    out += [_case("lap7_33x4x9", "greedy", "lap7", "central", variant="chunked"), _case("lap7_33x4x9", "greedy", "lap7", "forward", variant="colorrange")]
    # colourings on the medium pattern: more than 8 colours, columns without a colour, every column one colour (-> the plain kernel)
    for route in ("win", "rows", "ents", "jit", "terms"):
        out += [_case("random_band", "many", route, "forward"), _case("random_band", "none5", route, "central")]
    out += [_case("random_band", "ones", "cols", "forward"), _case("random_band", "ones", "cols", "central", dir=1.0, family="signed_zeros"),
            _case("random_band", "ones", "jit", "forward", dir=-1.0, family="signed_zeros", launch="cols"),
            _case("lap7_33x4x9", "ones", "lap7", "forward", launch="cols"), _case("lap7_33x4x9", "many", "lap7", "central"),
            _case("lap7_33x4x9", "none5", "lap7", "forward", dir=-1.0)]
    # rectangular patterns: the plain column kernel only
    for pat in ("wide", "tall"):
        for dtype in ("f64", "f32"):
            out += [_case(pat, "greedy", "cols", "forward", dtype=dtype), _case(pat, "none5", "cols", "central", dtype=dtype)]
        out.append(_case(pat, "greedy", "jit", "forward", dir=-1.0, launch="cols"))
    # rows longer than a row-wise tile's staged run
    for route in ("win", "rows", "terms"):
        for dtype in ("f64", "f32"):
            if dtype == "f32" and route.startswith("terms"):
                continue
            out += [_case("rows12", "greedy", route, "forward", dtype=dtype), _case("rows12", "greedy", route, "central", dtype=dtype)]
    # the edge patterns: ordinary, signed_zeros (dir = -1), nan_inf
    for fam, (fdtype, dir) in zip(EDGE_FAMILIES, (("central", 1.0), ("forward", -1.0), ("forward", 1.0))):
        for route in ("win", "rows", "ents", "jit", "terms"):
            out.append(_case("ragged400", "greedy", route, fdtype, dir=dir, family=fam))
        out.append(_case("ragged400", "invalid6" if fam == "nan_inf" else "ones", "cols", fdtype, dir=dir, family=fam))
        for n in (1, 2, 3) if fam != "nan_inf" else ():
            # (N = 1 and N = 3 are diagonals -- reach 0: the plain kernel; N = 2 is full, with a verified colouring and a reach of 1)
            out += [_case("tiny_%d" % n, "greedy", "win" if n == 2 else "cols", fdtype, dir=dir, family=fam),
                    _case("tiny_%d" % n, "greedy", "jit", fdtype, dir=dir, family=fam, launch=None if n == 2 else "cols")]
        if fam != "nan_inf":          # (the full 2 x 2 pattern through the row-wise routes: rows of two entries, one tile, one wavefront)
            out += [_case("tiny_2", "greedy", route, fdtype, dir=dir, family=fam) for route in ("rows", "ents", "terms")]
        for pat in ("lap7_7x5x3", "lap7_1x1x40"):
            out.append(_case(pat, "small" if fam == "nan_inf" else "greedy", "lap7", fdtype, dir=dir, family=fam))
    out += [_case("ragged400", "greedy", "win", "forward", dtype="f32"), _case("ragged400", "greedy", "rows", "central", dtype="f32"),
            _case("lap7_7x5x3", "greedy", "lap7", "central", dtype="f32"), _case("lap7_1x1x40", "ones", "lap7", "forward", launch="cols")]
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


CASES = _build_cases()


def np_dtype(case):
    return np.float64 if case["dtype"] == "f64" else np.float32


def inputs(case):
    """Everything a run of the case needs on the host: M, N, colptr, rowval, colors, c0, C, x, rel, ab, f (the model's residual), f_in."""
    M, N, colptr, rowval = pattern(case["pattern"])
    colors = colouring(case["pattern"], case["colouring"])
    dtype = np_dtype(case)
    C = int(colors.max())
    x, rel, ab = operands(case, colors)
    f_in = None
    if case["variant"] == "f_in":
        f_in = (np.random.default_rng(N).random(M) - 0.5).astype(dtype)         # any values: the subtrahend as it is given
    f = X.fixture("lap7", *LAP7[case["pattern"]]) if case["fixture"] == "lap7" else X.fixture("sparse", M, N, colptr, rowval)
    return dict(M=M, N=N, colptr=colptr, rowval=rowval, colors=colors, c0=colors - 1, C=C, x=x, rel=rel, ab=ab, dtype=dtype, f=f, f_in=f_in)


def layout(case, inp, part=None):
    """D -> [the array the case's destination holds]; part = (c_lo, c_hi): a colour-owning plan's share (zeros elsewhere)."""
    cp = inp["colptr"]
    if case["variant"] == "colwindow":
        a, b = COL_WINDOW
        return lambda D: [X.to_csc(D, inp["c0"], cp, inp["rowval"])[cp[a] - 1:cp[b] - 1]]
    if part is not None:
        c0 = np.where((inp["c0"] >= part[0]) & (inp["c0"] < part[1]), inp["c0"], -1)
        return lambda D: [X.to_csc(D, c0, cp, inp["rowval"])]
    return lambda D: [X.to_csc(D, inp["c0"], cp, inp["rowval"])]


def model(case):
    """The model's own answer (its own step sizes): (stored values, eps, scaled)."""
    inp = inputs(case)
    eps, scaled = X.epsilons(inp["x"], inp["c0"], inp["C"], case["fdtype"], relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"],
                             dtype=inp["dtype"])
    D = X.colour_values(inp["f"], inp["x"], inp["c0"], inp["C"], eps, case["fdtype"], f_in=inp["f_in"])
    return layout(case, inp)(D)[0], eps, scaled


def model_key(case):
    """Cases with equal keys have the same model answer (the route and the call form do not enter it)."""
    v = case["variant"] if case["variant"] in ("colwindow", "f_in") else None
    return (case["pattern"], case["colouring"], case["fixture"], case["fdtype"], case["dir"], case["dtype"], case["family"], v)


def div_sides(case):
    """The quotients of the case's stored entries, sorted by the two fall-back rules of fd_div_shared (include/fdjac_device.h, Float64)
    on the model's own numerators a and divisors b (b = eps_c, central: 2 eps_c; y = 1 / b):
      rule3   (a, b, y)        Markstein product iff |a y| and |a| both lie in [2^-900, 2^900] -- what every store route calls
      rule4   (a, b, y, b_ok)  Markstein product iff |b| in [2^-100, 2^100] and |a| in [2^-800, 2^800]
    Returns {"rule3": (n_product, n_division), "rule4": (...)} over the entries of coloured columns."""
    inp = inputs(case)
    T = inp["dtype"]
    eps, _ = X.epsilons(inp["x"], inp["c0"], inp["C"], case["fdtype"], relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"], dtype=T)
    x, c0, f = inp["x"], inp["c0"], inp["f"]
    with np.errstate(all="ignore"):
        A = np.empty((inp["C"], inp["M"]), T)
        base = None
        if case["fdtype"] == "forward":
            base = f(x) if inp["f_in"] is None else inp["f_in"]
        for c in range(inp["C"]):
            e = T(eps[c])
            z = np.copysign(T(0), e)
            m = c0 == c
            xp = np.where(m, x + e, x + z)
            A[c] = f(xp) - (base if base is not None else f(np.where(m, x - e, x - z)))
        cols = np.repeat(np.arange(inp["N"]), np.diff(inp["colptr"]))
        ok = c0[cols] >= 0
        a = np.abs(A[c0[cols[ok]], inp["rowval"][ok] - 1].astype(np.float64))
        b = np.abs(eps[c0[cols[ok]]].astype(np.float64)) * (2.0 if case["fdtype"] == "central" else 1.0)
        q0 = np.abs(a * (1.0 / b))
        r3 = (q0 >= 2.0 ** -900) & (q0 <= 2.0 ** 900) & (a >= 2.0 ** -900) & (a <= 2.0 ** 900)
        r4 = (b >= 2.0 ** -100) & (b <= 2.0 ** 100) & (a >= 2.0 ** -800) & (a <= 2.0 ** 800)
    return {"rule3": (int(r3.sum()), int((~r3).sum())), "rule4": (int(r4.sum()), int((~r4).sum())),
            "b": (float(b.min()), float(b.max())) if b.size else (0.0, 0.0)}
