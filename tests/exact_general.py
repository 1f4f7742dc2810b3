"""The cases of tests/test_gpu_exact_general.py: the hand-over path (k_perturb -> plain f! -> k_decompress_*) on GENERAL CSC patterns
against the exact host model (tests/exact_model.py), with the one residual the library ships for any pattern (FD_F_SPARSE).  Pure
numpy -- patterns, colourings, operands, the table of cases and the model's answer for each of them -- so that the CPU suite
(tests/test_exact_model.py) can evaluate every GPU case's inputs with the model alone.  Test infrastructure only.

  patterns     random_band (6 rows per column within +-300), ragged (4500 x 4000: empty rows, every seventh column empty, one dense row
               of 3000 entries), wide (300 x 5000), tall (5000 x 300), lap5 (the 5-point grid 70 x 40 as a general pattern: stride 70
               >= 64, 2800 >= 1024 columns, >= 8192 entries -- what try_window2d_plan asks for), tiny_N (N = 1, 2, 3, 65, 257)
  colourings   greedy   color_model.greedy: valid, NOT cyclic (random_band: more than kRegColors = 8 colours -- per-colour lists)
               none5    the same with 5 columns set to 0 (no colour: zeros are stored)
               stencil  (lap5 only) the grid's own five colours ((i + 2 j) mod 5: valid, not cyclic in the column index), and
                        stencil_none5 -- the greedy colouring of the grid has 10 colours, more than a row-window tile can hold
               invalid  the greedy colours folded into 5 (columns that share a row meet in one colour), one more pair of columns of
                        one row given one colour, and every 97th column moved to a sixth, small colour -- at most 6 colours: the
                        register reduction's CYC = false instantiation with its defined summation order, and few enough colours
                        per tile for the row-window kernels (a tile holds at most kWinMaxCol = 8 consecutive colours: the greedy colourings
                        of random_band, 19 colours, and of the grid, 10, cannot take them)
  operands     the families of tests/exact_operands.py (`cancel`, `few_huge` and `nan_inf` choose their columns by the case's own
               colour vector, not by the column index: the colourings here are not cyclic); phi is quadratic, so `num_2p800` / `huge_range` would overflow every row:
               `few_huge` instead (8 columns of one colour hold +-1e160..1e300: that colour's sum of squares overflows -> the scaled
               norm; only the rows those columns enter go non-finite).  `nan_inf` puts its NaN into the SMALLEST colour class and
               +Inf / -Inf into the second smallest (into the smallest too where the two together hold more than 5 % of the columns):
               a NaN / Inf coordinate makes its whole colour's step size and values non-finite, and at least 90 % of every case's
               stored values must stay finite for the comparison to mean something."""
import functools

import numpy as np

import color_model
import csc_solve_model
import exact_model as X
from exact_operands import operands as _operands
from finitediff_jl_amd import patterns as P

FAMILIES = ["ordinary", "signed_zeros", "cancel", "eps_2p100_in", "eps_2p100_out", "eps_2m100_in", "eps_2m100_out", "tiny_1e-200",
            "subnormal", "nan_inf", "few_huge"]
TINY = (1, 2, 3, 65, 257)
MIN_FINITE = 0.9


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(M, N, colptr, rowval), 1-based int64."""
    if name in ("random_band", "random_band600"):
        n = 6000 if name == "random_band" else 600
        cp, rv, _n = csc_solve_model.random_band_pattern(n, 300, 6, 11)
        return n, n, cp + 1, rv + 1
    if name == "ragged":
        return _ragged(4500, 4000, 2222, 3000, 12)
    if name == "wide":
        M, N = 300, 5000
        return (M, N) + color_model.random_band(M, N, 3, 10, 13)
    if name == "tall":
        M, N = 5000, 300
        return (M, N) + color_model.random_band(M, N, 36, 60, 14)      # (~9000 entries: the sorted kernel needs 4 tiles of 2048)
    if name == "lap5":
        return (2800, 2800) + P.lap5_csc(70, 40)
    if name.startswith("tiny_"):
        n = int(name[5:])
        j = np.arange(n)
        rows = np.sort(np.stack([j, (7 * j + 3) % n], axis=1), axis=1)          # 2 entries per column (1 where both coincide)
        keep = np.ones_like(rows, bool)
        keep[:, 1] = rows[:, 1] != rows[:, 0]
        colptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64) + 1
        return n, n, colptr, (rows[keep] + 1).astype(np.int64)
    raise ValueError(name)


def _ragged(M, N, dense_row, dense_len, seed):
    rng = np.random.default_rng(seed)
    j = np.arange(N)
    centre = (j * M) // N
    rows = centre[:, None] + rng.integers(-40, 41, size=(N, 3))
    live = j % 7 != 3                                                           # every seventh column is empty
    ok = (rows >= 0) & (rows < M) & (rows % 5 != 1) & (rows != dense_row) & live[:, None]     # rows = 1 mod 5 stay empty
    cols = np.broadcast_to(j[:, None], rows.shape)[ok]
    dense_cols = np.sort(rng.choice(np.nonzero(live)[0], size=dense_len, replace=False))
    key = np.unique(np.concatenate([cols * M + rows[ok], dense_cols * M + dense_row]))
    c, r = key // M, key % M
    colptr = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=N))]).astype(np.int64) + 1
    return M, N, colptr, (r + 1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def colouring(pname, kind):
    """The colour vector (int64, 1-based, 0 = no colour) of pattern `pname`."""
    M, N, colptr, rowval = pattern(pname)
    if kind == "greedy":
        return color_model.greedy(M, N, colptr, rowval)
    if kind in ("stencil", "stencil_none5"):                                    # the grid's own 5 colours (valid, not cyclic in the column index)
        assert pname == "lap5"
        g = P.lap5_colors(70, 40)
        if kind == "stencil_none5":
            g[np.unique([N // 7, N // 3, N // 2, (2 * N) // 3, N - 1])] = 0
        return g
    g = colouring(pname, "greedy").copy()
    if kind == "none5":
        g[np.unique([N // 7, N // 3, N // 2, (2 * N) // 3, N - 1])] = 0
        return g
    if kind == "invalid":
        g = (g - 1) % 5 + 1
        g[11::97] = 6
        _cp, _rows, row_ptr, row_cols = color_model._transpose(M, colptr, rowval, 1)
        r = int(np.nonzero(np.diff(row_ptr) >= 2)[0][0])                        # the first row that two columns share
        a, b = row_cols[row_ptr[r]], row_cols[row_ptr[r] + 1]
        g[b] = g[a]
        return g
    raise ValueError(kind)


def operands(family, pname, colors, dtype, seed, N=None):
    """(x, relstep, absstep) of the family on the pattern's columns (N given: a pattern of another table, tests/exact_store_cases.py)."""
    N = pattern(pname)[1] if N is None else N
    C = int(colors.max())
    if family not in ("nan_inf", "few_huge", "cancel"):
        return _operands(family, N, C, dtype, seed)
    x, rel, ab = _operands("ordinary", N, C, dtype, seed)
    size = np.bincount(colors, minlength=C + 1)[1:].astype(np.int64)
    if family == "cancel":          # the columns of ONE colour (the second) hold 1e30: every x + eps is absorbed -- zero numerators
        rng = np.random.default_rng(seed + 2)
        k = np.nonzero(colors == min(2, C))[0]
        x[k] = 1e30 * (1 + rng.random(k.size))
        return x, 1e-30, 1e-30
    if family == "few_huge":
        rng = np.random.default_rng(seed + 1)
        k = np.nonzero(colors == int(np.argmax(size)) + 1)[0][:8]               # 8 columns of the largest colour class
        x[k] = 10.0 ** rng.uniform(160, 300, k.size) * np.where(rng.random(k.size) < 0.5, -1, 1)
        return x, rel, ab
    order = np.argsort(size + np.where(size == 0, N + 1, 0), kind="stable")     # smallest non-empty class first
    first = np.nonzero(colors == order[0] + 1)[0]
    x[first[0]] = np.nan
    # (+Inf / -Inf get a colour of their own only where the two classes together hold at most 5 % of the columns; else they join the NaN's)
    own = C >= 2 and size[order[1]] >= 2 and size[order[0]] + size[order[1]] <= 0.05 * N
    second = np.nonzero(colors == order[1] + 1)[0] if own else first[1:]
    if second.size >= 2:
        x[second[0]] = np.inf
        x[second[-1]] = -np.inf
    return x, rel, ab


# ---- the table of cases --------------------------------------------------------------------------------------------------------------
def _case(pat, col, kernel, fdtype, dir=1.0, dtype="f64", family="ordinary", variant=None, tile=None):
    cid = "-".join([pat, col, kernel + (str(tile) if tile else ""), fdtype + ("m" if dir < 0 else ""), dtype, family] +
                   ([variant] if variant else []))
    return dict(id=cid, pattern=pat, colouring=col, kernel=kernel, fdtype=fdtype, dir=dir, dtype=dtype, family=family, variant=variant,
                tile=tile)


def _build_cases():
    out = []
    # the gather kernels on every pattern; the three colourings, both difference types and dir = -1 go round
    for pat in ("random_band", "wide", "tall", "lap5", "tiny_65", "tiny_257"):
        out += [_case(pat, "greedy", "list", "forward"), _case(pat, "none5", "list", "central"),
                _case(pat, "invalid", "list", "forward", dir=-1.0), _case(pat, "greedy", "sorted", "central"),
                _case(pat, "none5", "sorted", "forward", dir=-1.0), _case(pat, "invalid", "sorted", "central")]
    # (ragged: a valid colouring has one colour per column of the dense row -- 3000 evaluations of f; the cheap invalid one elsewhere)
    out += [_case("ragged", "greedy", "list", "forward"), _case("ragged", "invalid", "list", "central"),
            _case("ragged", "none5", "sorted", "central"), _case("ragged", "invalid", "sorted", "forward", dir=-1.0)]
    for n in (1, 2, 3):
        out += [_case("tiny_%d" % n, "greedy", "list", "forward", dir=-1.0), _case("tiny_%d" % n, "greedy", "sorted", "central")]
    # the row-window kernel at its three tile sizes, the 2-D tiles
    for tile in (512, 1024, 2048):
        out += [_case("random_band", "invalid", "window", "forward", tile=tile), _case("random_band", "invalid", "window", "central", tile=tile),
                _case("lap5", "stencil", "window", "forward", dir=-1.0, tile=tile), _case("lap5", "stencil_none5", "window", "central", tile=tile),
                _case("lap5", "invalid", "window", "forward", tile=tile)]
    out += [_case("lap5", "stencil", "window2d", "forward"), _case("lap5", "stencil", "window2d", "central"),
            _case("lap5", "stencil_none5", "window2d", "forward", dir=-1.0), _case("lap5", "invalid", "window2d", "central")]
    # Float32: list and window
    for pat in ("random_band", "lap5"):
        out += [_case(pat, "greedy", "list", "forward", dtype="f32"), _case(pat, "invalid", "list", "central", dtype="f32"),
                _case(pat, "invalid", "window", "forward", dir=-1.0, dtype="f32"), _case(pat, "invalid", "window", "central", dtype="f32")]
    # destinations and call forms
    for pat in ("random_band600", "wide"):
        out += [_case(pat, "greedy", "list", "forward", variant="dense"), _case(pat, "none5", "list", "central", variant="dense"),
                _case(pat, "invalid", "list", "forward", dir=-1.0, variant="dense")]
    out += [_case("random_band", "greedy", "list", "central", variant="chunked"), _case("random_band", "invalid", "window", "forward", variant="chunked"),
            _case("random_band", "greedy", "list", "forward", variant="colwindow"), _case("random_band", "invalid", "window", "central", variant="colwindow"),
            # (the device builder describes one-window tiles only: random_band's tiles need the host's clustering, so it builds index lists --
            #  colour-sorted tiles, the storage order being a scattered gather; no switch is forced)
            _case("random_band", "invalid", "auto", "forward", variant="device"), _case("random_band", "greedy", "auto", "central", variant="device"),
            _case("lap5", "stencil", "window2d", "central", variant="device"), _case("lap5", "stencil_none5", "window2d", "forward", variant="device"),
            _case("random_band", "greedy", "list", "forward", variant="f_in"), _case("random_band", "invalid", "window", "forward", dir=-1.0, variant="f_in"),
            _case("random_band", "none5", "sorted", "forward", variant="f_in")]
    # the operand families
    for fam in FAMILIES:
        if fam == "ordinary":
            continue
        for fdtype in ("forward", "central"):
            out += [_case("random_band", "greedy", "list", fdtype, family=fam), _case("random_band", "invalid", "window", fdtype, family=fam),
                    # (nan_inf needs a small colour class to poison: the grid's own five classes hold 20 % of the columns each)
                    _case("lap5", "stencil" if fdtype == "forward" and fam != "nan_inf" else "invalid", "window2d", fdtype, family=fam)]
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


COL_WINDOW = (1235, 5000)          # (an odd first column)
CASES = _build_cases()


def np_dtype(case):
    return np.float64 if case["dtype"] == "f64" else np.float32


def inputs(case):
    """Everything a run of the case needs on the host: M, N, colptr, rowval, colors, c0, C, x, rel, ab, f (the model's residual), f_in."""
    M, N, colptr, rowval = pattern(case["pattern"])
    colors = colouring(case["pattern"], case["colouring"])
    dtype = np_dtype(case)
    C = int(colors.max())
    x, rel, ab = operands(case["family"], case["pattern"], colors, dtype, 7 * N + C)
    f_in = None
    if case["variant"] == "f_in":
        f_in = (np.random.default_rng(N).random(M) - 0.5).astype(dtype)         # any values: the subtrahend as it is given
    return dict(M=M, N=N, colptr=colptr, rowval=rowval, colors=colors, c0=colors - 1, C=C, x=x, rel=rel, ab=ab, dtype=dtype,
                f=X.fixture("sparse", M, N, colptr, rowval), f_in=f_in)


def layout(case, inp):
    """D -> [the array the case's destination holds]."""
    if case["variant"] == "dense":
        return lambda D: [X.to_dense(D, inp["c0"], inp["colptr"], inp["rowval"], inp["M"], inp["N"])]
    if case["variant"] == "colwindow":
        a, b = COL_WINDOW
        cp = inp["colptr"]
        return lambda D: [X.to_csc(D, inp["c0"], cp, inp["rowval"])[cp[a] - 1:cp[b] - 1]]
    return lambda D: [X.to_csc(D, inp["c0"], inp["colptr"], inp["rowval"])]


def model(case, colour_values=X.colour_values, epsilons=X.epsilons):
    """The model's own answer (its own step sizes): (stored values, eps, scaled)."""
    inp = inputs(case)
    eps, scaled = epsilons(inp["x"], inp["c0"], inp["C"], case["fdtype"], relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"],
                           dtype=inp["dtype"])
    D = colour_values(inp["f"], inp["x"], inp["c0"], inp["C"], eps, case["fdtype"], f_in=inp["f_in"])
    return layout(case, inp)(D)[0], eps, scaled


def model_key(case):
    """Cases with equal keys have the same model answer (the kernel, the tile and the call form do not enter it)."""
    v = case["variant"] if case["variant"] in ("dense", "colwindow", "f_in") else None
    return (case["pattern"], case["colouring"], case["fdtype"], case["dir"], case["dtype"], case["family"], v)
