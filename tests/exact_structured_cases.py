"""The cases of tests/test_gpu_exact_structured.py: the routes that write the STRUCTURED storages -- BandedMatrix data and the band as
CSC (hand-over: k_decompress_banded / the window kernel; storing launch: fd_band_store_cols<L, U>), BlockBandedMatrix data (hand-over:
k_decompress_colrange_wg, paired and scalar; storing launch: fd_colrange_store_cols) and BandedBlockBandedMatrix data (hand-over:
k_decompress_bbb; storing launches: fd_bbb_store_cols, k_f_stencil5_store_bbb) -- against the exact host model (tests/exact_model.py).
Pure numpy, so that the CPU suite (tests/test_exact_structured_cpu.py) evaluates every case with the model alone: the finite share,
the sides of fd_div_shared's fall-back rules, the families' edges and the model mutations.  Test infrastructure only.

  layouts      band      BandedMatrix data (l + u + 1) x N (square), fixture BandF / BandSign
               bandcsc   the same band as SparseMatrixCSC nzval (the storing launch up to l + u = 8; wider: the column store)
               blocks    BlockBandedMatrix data, any block sizes, block bandwidths (bl, bu), fixture BlockRat / BlockSign
               bbb       BandedBlockBandedMatrix data of an nx x ny grid (ny blocks of nx, block bandwidths (1, 1), sub-bandwidths
                         (reach, reach)), fixture GridNL; with reach = 1 also the built-in 5-point families lap5 / lap5_nl; "ragged":
                         non-uniform blocks (hand-over only)
  routes       store     plan.set_lazy(functor): the storing launch where the plan offers it -- `store` says whether it must (False:
                         the plan or the launcher declines and the hand-over path runs; the GPU test asserts either)
               handover  no lazy launcher: k_perturb, the plain f!, the layout's decompression kernel
  colourings   own (the layout's valid colouring; band: cyclic with a shift), rev (band: valid, NOT cyclic), invalid (columns that share
               a row share a colour: the model promises the COLOUR's point), missing (a few columns without a colour)
  variants     f_in (f(x) with every seventh entry changed: subtracted as given), steps (relstep 1e-3, absstep 0), colwindow (band:
               a column window), chunked (blocks: eight colours at a time, so that c_lo > 0 runs), scalar (blocks hand-over:
               a destination that is only 8-byte aligned, which keeps k_decompress_colrange_wg off its paired form)
  operands     the families of tests/exact_operands.py.  LEFT OUT: huge_range and f32_huge (every fixture is at least quadratic in x:
               each poisoned coordinate overflows every row that reads it -- a fifth of the band's columns, every block row).
               RESIZED: num_2p800 as in tests/exact_store_cases.py (|x| = 10^U(100, 150), absstep 1e136; the cubic BlockRat:
               10^U(60, 100), 1e86): the numerators pass 2^800 and stay finite.  num_2m900 is that table's own family (subnormal
               coordinates, absstep 1e-290).  nan_inf on block-banded storage: a NaN coordinate poisons its block's sum, hence three
               block rows; on the 9 x 32 shape that is a third of the stored values, so nan_inf runs on 48 blocks of 24 with NaN, +Inf and
               -Inf all in block 0 (two block rows of 48, three colours of 72).  Elsewhere the three share ONE small colour class
               (nan_colouring): a NaN coordinate makes its colour's step NaN, and a cyclic colouring of at most 8 classes -- all a
               BandedMatrix plan's storing launch takes -- would lose an eighth of the columns to it.
MIN_FINITE: the model alone keeps at least 90 % of every case's stored values finite (asserted on the CPU, a condition of the case)."""
import functools

import numpy as np

import exact_model as X
from exact_operands import operands as _operands
from finitediff_jl_amd import patterns as P

MIN_FINITE = 0.9
FAMILIES64 = ["ordinary", "signed_zeros", "cancel", "eps_2p100_in", "eps_2p100_out", "eps_2m100_in", "eps_2m100_out", "num_2p800",
              "num_2m900", "tiny_1e-200", "subnormal", "nan_inf"]
FAMILIES32 = ["ordinary", "signed_zeros", "f32_subnormal", "nan_inf"]
EDGE_FAMILIES = ["ordinary", "signed_zeros", "nan_inf"]
DIV_FAMILIES = ["eps_2p100_in", "eps_2p100_out", "eps_2m100_in", "eps_2m100_out", "num_2p800", "num_2m900", "tiny_1e-200", "subnormal"]
LEFT_OUT = {"huge_range": "every fixture is at least quadratic: a poisoned colour overflows every row that reads it",
            "f32_huge": "the same in Float32 (|x| = 3e38)"}
DIRS = (("forward", 1.0), ("forward", -1.0), ("central", 1.0))
BAND_LU = [(2, 2), (3, 3), (2, 1), (1, 0), (0, 1), (0, 0), (4, 4), (5, 4)]
BLOCK_SHAPES = [(1, 1), (1, 2), (2, 3), (3, 8), (5, 7), (9, 32), (4, 70), (33, 2)]
RAGGED_BLOCKS = (3, 1, 8, 2, 5, 32, 4)
GRIDS = [(1, 1, 1), (2, 1, 1), (3, 2, 1), (5, 3, 2), (4, 4, 3), (23, 17, 3), (64, 5, 2), (40, 30, 1)]
RAGGED_GRID = (5, 3, 7, 4)             # block sizes of the non-uniform BBB case (reach 2)
MID = {"band": ((2, 2), 1025), "bandcsc": ((2, 2), 1025), "blocks": (9, 32), "bbb": (23, 17, 3)}
NAN_BLOCKS = (48, 24)
CHUNK_COLOURS = 8


def band_sizes(l, u):
    return sorted({1, 2, max(l + u, 1), l + u + 2, 127, 128, 129, 511, 512, 513, 1025})


def band_store_offered(layout, l, u, N, C, cyclic, missing):
    """Does a plan with a FD_LAZY_CAP_STORE functor take the storing launch (csrc/fdjac_plan_list.hip: store_caps_implicit_band,
    try_store_plan_csc; csrc/fdjac_jit.hip: band_function)?  BandedMatrix: cyclic colours, l + u + 1 <= C <= 8 (the register reduction
    recognises them); CSC: at least four columns, cyclic, C >= l + u + 1, l + u <= 8."""
    if not cyclic or missing or C < l + u + 1 or l + u > 8:
        return False
    return C <= 8 if layout == "band" else N >= 4


def _case(layout, shape, route, fdtype, dir=1.0, dtype="f64", family="ordinary", colouring="own", variant=None, fixture=None, store=None,
          shift=0):
    fixture = fixture or {"band": "band", "bandcsc": "band", "blocks": "blockrat", "bbb": "grid"}[layout]
    flat = lambda v: [v] if not isinstance(v, tuple) else [w for t in v for w in flat(t)]
    sname = "x".join(str(v) for v in flat(shape))
    cid = "-".join([layout, sname, fixture, colouring + (str(shift) if shift else ""), route, fdtype + ("m" if dir < 0 else ""), dtype, family]
                   + ([variant] if variant else []))
    c = dict(id=cid, layout=layout, shape=shape, route=route, fdtype=fdtype, dir=dir, dtype=dtype, family=family, colouring=colouring,
             variant=variant, fixture=fixture, shift=shift)
    if store is None:
        valid = colouring in ("own", "cyc40", "wide")
        store = route == "store" and valid and fdtype != "complex" and variant != "f_in"
        if layout.startswith("band") and store:
            (l, u), N = shape
            a, b = col_window(c) if variant == "colwindow" else (0, N)
            store = band_store_offered(layout, l, u, b - a, 40 if colouring == "cyc40" else l + u + 1, True, False)
        if layout == "blocks":          # (a compiled functor serves all three fdtypes; a caller's f_in sends forward differences to the hand-over)
            store = route == "store" and valid and variant != "f_in"
        if layout == "bbb":             # (fd_bbb_store_cols writes the zeros of a column without a colour itself: such a colouring keeps the launch)
            store = route == "store" and (valid or colouring == "missing") and variant != "f_in" and shape != "ragged"
    c["store"] = bool(store)
    return c


def nan_colouring(layout, fam):
    """nan_inf: a NaN coordinate makes its whole colour's step NaN, so the three non-finite coordinates share ONE colour, and that colour
    is a small class: 40 cyclic colours on the band (a BandedMatrix plan then declines the storing launch -- more than 8 -- and the band
    as CSC takes it), four times the layout's own number on BBB storage.  Block-banded: the layout's own (72 classes at 48 x 24)."""
    if fam != "nan_inf" or layout == "blocks":
        return "own"
    return "cyc40" if layout.startswith("band") else "wide"


def col_window(case):
    N = case["shape"][1]
    return (N // 3) | 1, (2 * N // 3) & ~1          # (an odd first column, an even end)


def _build_cases():
    out = []
    # ---- every route x the operand matrix at one mid-size shape per layout --------------------------------------------------------------
    for layout in ("band", "bandcsc", "blocks", "bbb"):
        for route in ("store", "handover"):
            if layout == "bandcsc" and route == "handover":
                continue                   # (the hand-over of a CSC band is the general-pattern anchor: tests/test_gpu_exact_general.py)
            for fam in FAMILIES64:
                shape = NAN_BLOCKS if (layout == "blocks" and fam == "nan_inf") else MID[layout]
                for fdtype, dir in DIRS:
                    if dir < 0 and fam not in EDGE_FAMILIES:
                        continue
                    out.append(_case(layout, shape, route, fdtype, dir=dir, family=fam, shift=1 if layout.startswith("band") else 0,
                                     colouring=nan_colouring(layout, fam)))
                if fam in EDGE_FAMILIES and (layout == "blocks" or (layout == "band" and route == "handover")):
                    out.append(_case(layout, shape, route, "complex", family=fam, colouring=nan_colouring(layout, fam)))
            for fam in FAMILIES32:
                shape = NAN_BLOCKS if (layout == "blocks" and fam == "nan_inf") else MID[layout]
                out.append(_case(layout, shape, route, "central" if fam == "signed_zeros" else "forward", dtype="f32", family=fam,
                                 colouring=nan_colouring(layout, fam)))
            out.append(_case(layout, MID[layout], route, "forward", dir=-1.0, dtype="f32", family="signed_zeros"))
            # call forms: a caller's f_in (store route: the plan must take the hand-over), explicit steps
            out.append(_case(layout, MID[layout], route, "forward", variant="f_in"))
            out.append(_case(layout, MID[layout], route, "forward", dir=-1.0, family="signed_zeros", variant="f_in"))
            out.append(_case(layout, MID[layout], route, "forward", dir=-1.0, variant="steps"))
            out.append(_case(layout, MID[layout], route, "central", variant="steps"))
    # ---- the built-in 5-point families on BBB storage (k_f_stencil5_store_bbb), reach 1 ---------------------------------------------------
    for fam in FAMILIES64:
        for fdtype, dir in DIRS:
            if dir < 0 and fam not in EDGE_FAMILIES:
                continue
            out.append(_case("bbb", (40, 30, 1), "store", fdtype, dir=dir, family=fam, fixture="lap5_nl", colouring=nan_colouring("bbb", fam)))
    out += [_case("bbb", (40, 30, 1), "store", "forward", fixture="lap5"), _case("bbb", (40, 30, 1), "handover", "central", fixture="lap5"),
            _case("bbb", (40, 30, 1), "store", "forward", fixture="lap5_nl", variant="f_in")]
    # ---- shapes: the band ----------------------------------------------------------------------------------------------------------------------
    for k, (l, u) in enumerate(BAND_LU):
        for n, N in enumerate(band_sizes(l, u)):
            fdtype, dir = DIRS[(k + n) % 3]
            fam = EDGE_FAMILIES[n % 2]                           # ordinary / signed_zeros
            if N < l + u + 1:                                    # (fewer columns than colours: a cyclic colouring of N classes)
                out.append(_case("band", ((l, u), N), "handover", fdtype, dir=dir, family=fam, store=False))
                continue
            out.append(_case("band", ((l, u), N), "store", fdtype, dir=dir, family=fam, shift=(k + n) % (l + u + 1)))
            if N in (l + u + 2, 129, 513):
                out.append(_case("band", ((l, u), N), "handover", fdtype, dir=dir, family=fam, shift=1 if l + u else 0))
                out.append(_case("bandcsc", ((l, u), N), "store", fdtype, dir=dir, family=fam, shift=(k + n) % (l + u + 1)))
        out.append(_case("band", ((l, u), 513), "store", "central", dtype="f32", shift=u))
    for fdtype, dir in DIRS:
        out += [_case("band", ((2, 2), 513), "store", fdtype, dir=dir, colouring="rev"),
                _case("band", ((2, 2), 513), "handover", fdtype, dir=dir, colouring="invalid"),
                _case("band", ((2, 2), 513), "store", fdtype, dir=dir, colouring="invalid"),
                _case("band", ((2, 2), 1025), "store", fdtype, dir=dir, variant="colwindow", shift=3),
                _case("band", ((3, 3), 1025), "handover", fdtype, dir=dir, variant="colwindow", shift=2)]
    out.append(_case("band", ((2, 2), 513), "handover", "complex", colouring="rev"))
    # ---- shapes: block-banded ------------------------------------------------------------------------------------------------------------------
    for k, shape in enumerate(BLOCK_SHAPES + ["ragged"]):
        for n, (fdtype, dir) in enumerate(DIRS + (("complex", 1.0),)):
            fam = EDGE_FAMILIES[(k + n) % 2]
            for route in ("store", "handover"):
                out.append(_case("blocks", shape, route, fdtype, dir=dir, family=fam))
        out.append(_case("blocks", shape, "handover", "forward", variant="scalar"))
        out.append(_case("blocks", shape, "handover", "central", variant="f_in" if k % 2 else "scalar"))
    for shape in ((5, 7), "ragged", (9, 32)):
        for fdtype, dir in DIRS:
            out += [_case("blocks", shape, "handover", fdtype, dir=dir, colouring="missing"),
                    _case("blocks", shape, "store", fdtype, dir=dir, colouring="missing"),
                    _case("blocks", shape, "handover", fdtype, dir=dir, colouring="invalid")]
        out += [_case("blocks", shape, "store", "central", variant="chunked"), _case("blocks", shape, "handover", "forward", variant="chunked"),
                _case("blocks", shape, "store", "complex", variant="chunked"), _case("blocks", shape, "store", "central", dtype="f32"),
                _case("blocks", shape, "handover", "complex", dtype="f32")]
    for bw in ((2, 0), (0, 1)):
        for fdtype, dir in DIRS:
            out += [_case("blocks", ((5, 7), bw), route, fdtype, dir=dir) for route in ("store", "handover")]
    # ---- shapes: banded-block-banded -----------------------------------------------------------------------------------------------------------
    for k, shape in enumerate(GRIDS + ["ragged"]):
        for n, (fdtype, dir) in enumerate(DIRS):
            fam = EDGE_FAMILIES[(k + n) % 2]
            for route in ("store", "handover"):
                out.append(_case("bbb", shape, route, fdtype, dir=dir, family=fam))
        out.append(_case("bbb", shape, "handover", "forward", colouring="missing"))
        out.append(_case("bbb", shape, "store", "central", colouring="missing"))
        out.append(_case("bbb", shape, "handover", "forward", variant="f_in"))
    out += [_case("bbb", (23, 17, 3), "store", "central", dtype="f32"), _case("bbb", (64, 5, 2), "handover", "forward", dtype="f32")]
    # ---- the sign-sensitive fixtures at signed zeros: every route, both directions, central ----------------------------------------------------
    for fdtype, dir in DIRS:
        for route in ("store", "handover"):
            out += [_case("band", ((2, 2), 513), route, fdtype, dir=dir, family="signed_zeros", fixture="band_sign", shift=2),
                    _case("blocks", (5, 7), route, fdtype, dir=dir, family="signed_zeros", fixture="block_sign"),
                    _case("blocks", "ragged", route, fdtype, dir=dir, family="signed_zeros", fixture="block_sign")]
        out.append(_case("bandcsc", ((2, 2), 513), "store", fdtype, dir=dir, family="signed_zeros", fixture="band_sign", shift=2))
    seen = {}
    for c in out:                       # (a shape section repeats a few cases of the operand matrix at the mid-size shape: each once)
        seen.setdefault(c["id"], c)
    return list(seen.values())


def np_dtype(case):
    return np.float64 if case["dtype"] == "f64" else np.float32


def block_shape(case):
    """(block sizes, bl, bu) of a `blocks` case."""
    shape = case["shape"]
    if shape == "ragged":
        return np.array(RAGGED_BLOCKS, np.int64), 1, 1
    if isinstance(shape[1], tuple):
        (nb, bs), (bl, bu) = shape
        return np.full(nb, bs, np.int64), bl, bu
    return np.full(shape[0], shape[1], np.int64), 1, 1


@functools.lru_cache(maxsize=None)
def _layout(layout, shape):
    if layout == "blocks":
        bs, bl, bu = block_shape(dict(shape=shape))
        return P.BlockBandedLayout(bs, bl, bu)
    if shape == "ragged":
        return P.BandedBlockBandedLayout(np.array(RAGGED_GRID, np.int64), 1, 1, 2, 2)
    nx, ny, reach = shape
    return P.BandedBlockBandedLayout(np.full(ny, nx, np.int64), 1, 1, reach, reach)


def colours(case):
    """The colour vector (int64, 1-based, 0 = no colour)."""
    layout, kind = case["layout"], case["colouring"]
    if layout.startswith("band"):
        (l, u), N = case["shape"]
        W = min(l + u + 1, N)               # (fewer columns than the band is wide: N classes)
        j = np.arange(N, dtype=np.int64)
        if kind == "own":
            return (j + case["shift"]) % W + 1
        if kind == "cyc40":
            return (j + case["shift"]) % 40 + 1
        if kind == "rev":
            return W - (j % W)
        if kind == "invalid":
            return j % (W - 1) + 1
        raise ValueError(kind)
    lay = _layout(layout, case["shape"])
    g = lay.colors().copy()
    N = g.size
    if kind == "wide":      # (BBB: the layout's colouring over four times as many block classes -- still valid)
        w, sw = 4 * (lay.bl + lay.bu + 1), lay.lam + lay.mu + 1
        return np.concatenate([sw * (J % w) + (np.arange(b) % sw) + 1 for J, b in enumerate(lay.blk_sizes)]).astype(np.int64)
    if kind == "missing":
        g[np.unique([N // 7, N // 3, N // 2, (2 * N) // 3, N - 1])] = 0
    elif kind == "invalid":
        g = (g - 1) % max(int(g.max()) // 2, 1) + 1
    elif kind != "own":
        raise ValueError(kind)
    return g


def fixture(case):
    """(f, f on (re, im) pairs or None): the numpy restatements of the case's functor."""
    name, layout, shape = case["fixture"], case["layout"], case["shape"]
    if name in ("band", "band_sign"):
        (l, u), N = shape
        return X.band_f(N, l, u, sign=name == "band_sign"), (X.band_fc(N, l, u) if name == "band" else None)
    if name in ("blockrat", "block_sign"):
        bs, bl, bu = block_shape(case)
        return X.blockrat_f(bs, bl, bu, sign=name == "block_sign"), (X.blockrat_fc(bs, bl, bu) if name == "blockrat" else None)
    if name == "grid":
        if shape == "ragged":
            return ragged_grid_f(), None
        return X.grid_f(*shape), None
    if name in ("lap5", "lap5_nl"):
        nx, ny, _reach = shape
        return X.fixture(name, nx, ny), None
    raise ValueError(name)


def ragged_grid_f():
    """RaggedGrid (tests/jit_fixtures.py), the residual of the non-uniform BBB case: GridNL with reach 2 on grid rows of DIFFERENT
    lengths -- row k of block K, local index i: x_k x_k + the neighbours within 2 inside the block (0.5 / d west, (0.25 d east) x_k) +
    the coordinate with the same local index in block K - 1 + twice that of block K + 1 (where that block is long enough)."""
    bs = np.array(RAGGED_GRID, np.int64)
    off = np.concatenate([[0], np.cumsum(bs)])
    blk = np.repeat(np.arange(bs.size), bs)
    loc = np.arange(off[-1]) - off[blk]
    n = bs[blk]

    def f(x):
        x = np.asarray(x)
        T = x.dtype.type
        k = np.arange(x.size)
        zero = np.zeros_like(x)
        with np.errstate(all="ignore"):
            s = x * x
            for d in (1, 2):
                hw, he = loc - d >= 0, loc + d < n
                s = s + np.where(hw, T(0.5 / d) * x[np.where(hw, k - d, k)], zero)
                s = s + np.where(he, (T(0.25 * d) * x[np.where(he, k + d, k)]) * x, zero)
            hs = (blk > 0) & (loc < np.where(blk > 0, bs[np.maximum(blk - 1, 0)], 0))
            hn = (blk + 1 < bs.size) & (loc < np.where(blk + 1 < bs.size, bs[np.minimum(blk + 1, bs.size - 1)], 0))
            ks = np.where(hs, off[np.maximum(blk - 1, 0)] + loc, k)
            kn = np.where(hn, off[np.minimum(blk + 1, bs.size - 1)] + loc, k)
            s = s + np.where(hs, x[ks], zero)
            s = s + np.where(hn, T(2) * x[kn], zero)
        return s
    return f


def operands(case, N, C):
    dtype, fam = np_dtype(case), case["family"]
    seed = 7 * N + C
    if case["variant"] == "steps":
        x, _r, _a = _operands(fam, N, C, dtype, seed)
        return x, 1e-3, 0.0
    if fam == "num_2m900":
        x, _r, _a = _operands("subnormal", N, C, dtype, seed)
        return x, 1e-300, 1e-290
    if fam == "num_2p800":
        lo, hi, ab = (60, 100, 1e86) if case["fixture"].startswith(("block", "lap5")) else (100, 150, 1e136)       # (cubic / quadratic rows)
        rng = np.random.default_rng(seed)
        x = 10.0 ** rng.uniform(lo, hi, N) * np.where(rng.random(N) < 0.5, -1, 1)
        return x.astype(dtype), 1e-300, ab
    if fam == "nan_inf":
        x, rel, ab = _operands("ordinary", N, C, dtype, seed)
        if case["layout"] == "blocks":
            at = np.arange(3)                              # (all in block 0: two block rows are poisoned)
        elif case["layout"].startswith("band"):
            at = 40 * (N // 120) + 40 * np.arange(3)       # (one colour of the 40)
        else:
            nx, ny, reach = case["shape"]
            at = (ny // 2) * nx + 1 + (2 * reach + 1) * np.arange(3)      # (one grid row, one colour)
        x[at] = [np.nan, np.inf, -np.inf]
        return x, rel, ab
    return _operands(fam, N, C, dtype, seed)


def inputs(case):
    """Everything a run of the case needs on the host."""
    layout, shape = case["layout"], case["shape"]
    dtype = np_dtype(case)
    colors = colours(case)
    N = colors.size
    C = int(colors.max())
    x, rel, ab = operands(case, N, C)
    f, fc = fixture(case)
    f_in = None
    if case["variant"] == "f_in":
        with np.errstate(all="ignore"):
            f_in = f(x).copy()
        f_in[::7] = (f_in[::7] + dtype(0.5)) * dtype(1.25)       # (f(x) with every seventh entry changed)
    out = dict(N=N, M=N, colors=colors, c0=colors - 1, C=C, x=x, rel=rel, ab=ab, dtype=dtype, f=f, fc=fc, f_in=f_in)
    if layout.startswith("band"):
        (l, u), _N = shape
        out.update(l=l, u=u)
        if layout == "bandcsc":
            out["colptr"], out["rowval"] = P.banded_csc(N, N, l, u)
    else:
        out["lay"] = _layout(layout, shape)
    return out


def layout_fn(case, inp, outside=0.0, row_shift=0):
    """D -> the array the destination holds."""
    layout = case["layout"]
    c0 = inp["c0"]
    if layout == "band":
        l, u, N = inp["l"], inp["u"], inp["N"]
        a, b = col_window(case) if case["variant"] == "colwindow" else (0, N)
        W = l + u + 1
        return lambda D: X.to_banded_general(D, c0, N, N, l, u, outside, row_shift)[W * a:W * b]
    if layout == "bandcsc":
        return lambda D: X.to_csc(D, c0, inp["colptr"], inp["rowval"])
    if layout == "blocks":
        return lambda D: X.to_blockbanded(D, c0, inp["lay"])
    return lambda D: X.to_bandedblockbanded(D, c0, inp["lay"], outside, row_shift)


def library_zero(case):
    """The comparison uses the library's form of an unperturbed coordinate (x_i + (+0.0) whatever the sign of the step) instead of the
    model's x_i + copysign(0, eps_c): the sign-sensitive fixtures with dir = -1 -- the one place where the two differ and a stored bit
    can show it (the head of tests/test_gpu_exact_structured.py)."""
    return case["fixture"] in ("band_sign", "block_sign") and case["dir"] < 0 and case["fdtype"] == "forward"


MUTATIONS = ("plain_fx", "no_plus_zero", "unwritten_slot", "dir_on_quotient", "neighbour_eps", "row_off")


def model(case, mutation=None, inp=None):
    """The model's own answer (its own step sizes): (stored values, eps, scaled).  mutation: one of MUTATIONS -- a deliberately wrong
    model, for the CPU suite's check that a named case tells it apart."""
    inp = inp or inputs(case)
    T, C, c0, x = inp["dtype"], inp["C"], inp["c0"], inp["x"]
    fdtype, dir = case["fdtype"], case["dir"]
    if fdtype == "complex":
        eps, scaled = X.complex_epsilons(C, T), np.zeros(C, bool)
        if mutation == "neighbour_eps":
            return None
        D = X.colour_values_complex(inp["fc"], x, c0, C, eps)
    else:
        eps, scaled = X.epsilons(x, c0, C, fdtype, relstep=inp["rel"], absstep=inp["ab"], dir=1.0 if mutation == "dir_on_quotient" else dir, dtype=T)
        use = np.roll(eps, 1) if mutation == "neighbour_eps" else eps
        zero = "none" if mutation == "no_plus_zero" else "library" if library_zero(case) else "model"
        D = X.colour_values(inp["f"], x, c0, C, use, fdtype, f_in=None if mutation == "plain_fx" else inp["f_in"], zero=zero)
        if mutation == "dir_on_quotient" and fdtype == "forward":
            D = D * T(dir)
    kw = {}
    if mutation == "unwritten_slot":
        kw["outside"] = np.nan
    if mutation == "row_off":
        kw["row_shift"] = 1
    if kw and case["layout"] not in ("band", "bbb"):
        return None
    return layout_fn(case, inp, **kw)(D), eps, scaled


def div_sides(case, inp=None):
    """The two fall-back rules of fd_div_shared (include/fdjac_device.h; the restatement of tests/exact_store_cases.py) on the model's own
    numerators a and divisors b of the band's stored entries: {"rule3": (n_product, n_division)}.  The band kernel calls the
    three-argument form; the column-range and BBB kernels and all three hand-over kernels divide plainly."""
    inp = inp or inputs(case)
    T, C, c0, x, f = inp["dtype"], inp["C"], inp["c0"], inp["x"], inp["f"]
    eps, _ = X.epsilons(x, c0, C, case["fdtype"], relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"], dtype=T)
    central = case["fdtype"] == "central"
    with np.errstate(all="ignore"):
        A = np.empty((C, inp["N"]), T)
        base = None if central else (f(x) if inp["f_in"] is None else inp["f_in"])
        for c in range(C):
            e = T(eps[c])
            z = np.copysign(T(0), e)
            m = c0 == c
            A[c] = f(np.where(m, x + e, x + z)) - (base if base is not None else f(np.where(m, x - e, x - z)))
        cp, rv = P.banded_csc(inp["N"], inp["N"], inp["l"], inp["u"])
        cols = np.repeat(np.arange(inp["N"]), np.diff(cp))
        a = np.abs(A[c0[cols], rv - 1].astype(np.float64))
        b = np.abs(eps[c0[cols]].astype(np.float64)) * (2.0 if central else 1.0)
        q0 = np.abs(a * (1.0 / b))
        r3 = (q0 >= 2.0 ** -900) & (q0 <= 2.0 ** 900) & (a >= 2.0 ** -900) & (a <= 2.0 ** 900)
    return {"rule3": (int(r3.sum()), int((~r3).sum())), "a": (float(np.nanmin(a)), float(np.nanmax(a))), "b": (float(b.min()), float(b.max()))}


def model_key(case):
    """Cases with equal keys have the same model answer (the route does not enter it; of the variants only those that change operands or
    the destination do)."""
    v = case["variant"] if case["variant"] in ("colwindow", "f_in", "steps") else None
    return (case["layout"], str(case["shape"]), case["fixture"], case["colouring"], case["shift"], case["fdtype"], case["dir"], case["dtype"],
            case["family"], v)


CASES = _build_cases()
