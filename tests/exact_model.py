"""Exact host model of what the storing kernels promise (csrc/fdjac_f_*.hip, include/fdjac_device.h): the BITS of the plain
colour-by-colour evaluation of src/jacobians.jl:537-622, restated in vectorised numpy independently of the library.  Test
infrastructure only.

  step sizes   the masked sums of squares in the defined order (eps_order.masked_sumsq), then the step rule in the element type:
               max(relstep * abs(sqrt(norm)), absstep) [* dir] with Julia's NaN-propagating max; a colour whose plain sum overflowed,
               or underflowed while the relative term can still exceed absstep, takes the scaled norm sqrt(sum (x 2^-+600)^2) 2^+-600
               (its summation order is not defined: such step sizes are checked against mpmath, not bit for bit)
  points       colour c: the plus point is x + eps_c on the colour's coordinates and x + copysign(0, eps_c) elsewhere (Julia's
               eps * false); forward differences subtract f(x), central ones f at x - eps_c mask_c (x - copysign(0, eps_c) elsewhere)
  values       f in the element type, in the fixture's own operation order (csrc: tridiag_row, stencil5_row), the IEEE difference,
               the IEEE quotient by eps_c (central: by 2 eps_c)
  layout       CSC nzval, BandedMatrix data, Tridiagonal dl / d / du; uncoloured columns hold 0

The reference's in-place un-perturbation (x1 - eps mask after every colour) is NOT modelled: every colour starts from x.

The general-pattern anchor.  The hand-over path on ANY CSC pattern (k_perturb -> plain f! -> k_decompress_list / _sorted / _window /
_window2d) is what every "same bits" comparison of the store routes and of the decompression kernels ends in.  sparse_f restates the
one residual the library ships for any pattern (FD_F_SPARSE, SparseF::row in csrc/fdjac_functor_f.hip: f_r = sum over the pattern's
entries (r, j) of row r, ascending j, of w(r, j) phi(x_j), one IEEE operation at a time in a fixed order), so the model covers random
and rectangular patterns, empty rows and columns, greedy / invalid colourings and columns without a colour
(tests/exact_general.py holds the cases, tests/test_gpu_exact_general.py runs them); to_dense is the dense-J destination.

The complex step.  imag(f(x + i eps mask_c)) / eps with eps = eps(T) for every colour: the residuals restated on explicit (re, im)
pairs of real arrays (c_add ... c_div_s, tridiag_fc, stencil5_fc, lap7_fc, sparse_fc, colour_values_complex) in the operation order
of `cd` (csrc/fdjac_builtin_f.hip) and fd_cplx<T> (include/fdjac_device.h); an unperturbed coordinate's imaginary part is +0
(tests/exact_complex_cases.py holds the cases, tests/test_gpu_exact_complex.py runs them)."""
import numpy as np

import eps_order

F64 = np.float64


def default_relstep(fdtype, dtype=F64):
    e = np.finfo(dtype).eps
    return float(np.sqrt(np.dtype(dtype).type(e))) if fdtype == "forward" else float(np.cbrt(np.dtype(dtype).type(e)))


def rescale_exp(t, relstep, absstep, dtype=F64):
    """The exponent k of the scaled fallback (csrc/fdjac_internal.h, eps_rescale_exp), or 0: the plain sum stands."""
    if np.dtype(dtype) != np.dtype(F64):
        return 0                       # Float32 elements are summed in Float64: neither over- nor underflow can happen
    if t == np.inf:
        return -600
    if t < 2.0 ** -960 and absstep < relstep * 2.0 ** -240:
        return 600
    return 0


def jl_max(a, b):
    return a if (a > b or a != a) else b


def epsilons(x, colors0, C, fdtype, relstep=None, absstep=None, dir=1.0, dtype=F64):
    """(eps[C] in the element type, scaled[C]: the colour took the scaled fallback).  colors0: 0-based, < 0 = no colour."""
    T = np.dtype(dtype).type
    relstep = default_relstep(fdtype, dtype) if relstep is None else float(relstep)
    absstep = relstep if absstep is None else float(absstep)
    x = np.asarray(x, dtype=dtype)
    colors0 = np.asarray(colors0)
    with np.errstate(all="ignore"):
        tot = eps_order.masked_sumsq(x, colors0, C, dtype)
        out = np.empty(C, dtype=dtype)
        scaled = np.zeros(C, bool)
        for c in range(C):
            k = rescale_exp(tot[c], relstep, absstep, dtype)
            if k:
                y = x[colors0 == c].astype(F64) * 2.0 ** k
                nrm = np.sqrt(np.dot(y, y)) * 2.0 ** -k
                scaled[c] = True
            else:
                nrm = np.sqrt(tot[c])
            xs = np.abs(np.sqrt(T(nrm)))
            e = jl_max(T(relstep) * xs, T(absstep))
            if fdtype == "forward":
                e = e * T(dir)
            out[c] = e
    return out, scaled


# ---- the fixtures, in the operation order of csrc (every neighbour outside the domain is 0) ----
def tridiag_f(x, nl):
    T = x.dtype.type
    z = np.zeros(1, x.dtype)
    xm = np.concatenate([z, x[:-1]])
    xp = np.concatenate([x[1:], z])
    v = (xm - T(2) * x) + xp
    if nl:
        v = v + (x * x) * xp
    return v


def stencil5_f(x, nx, ny, nl):
    T = x.dtype.type
    g = x.reshape(ny, nx)
    z = np.zeros_like(g)
    w = z.copy(); w[:, 1:] = g[:, :-1]
    e = z.copy(); e[:, :-1] = g[:, 1:]
    s = z.copy(); s[1:, :] = g[:-1, :]
    n = z.copy(); n[:-1, :] = g[1:, :]
    v = (((w + e) + s) + n) - T(4) * g
    if nl:
        v = v + (g * g) * e
    return v.reshape(-1)


def lap7_f(x, nx, ny, nz):
    """FD_F_LAP7 (lap7_row in csrc/fdjac_functor_f.hip) in x's REAL element type: the six neighbours added in the order down, south,
    west, east, north, up (0 outside the grid), minus 6 times the centre, plus (centre * centre) * east.  (The complex step's form is
    lap7_fc below, on explicit (re, im) pairs: numpy's complex dtypes are not used for values.)"""
    T = x.dtype.type
    g = x.reshape(nz, ny, nx)
    d, s, w, e, n, u = (np.zeros_like(g) for _ in range(6))
    d[1:] = g[:-1]
    u[:-1] = g[1:]
    s[:, 1:] = g[:, :-1]
    n[:, :-1] = g[:, 1:]
    w[:, :, 1:] = g[:, :, :-1]
    e[:, :, :-1] = g[:, :, 1:]
    return (((((((d + s) + w) + e) + n) + u) - T(6) * g) + (g * g) * e).reshape(-1)


def sparse_f(M, N, colptr, rowval, dtype=F64):
    """FD_F_SPARSE (SparseF::row) in the element type: f_r = sum over the entries (r, j) of row r, ascending j, left to right, of
    w * (v + (q * v) * v) with v = x_j, w = 1 + ((r + 3 j) & 7) / 8 and q = 1 / 4 in the element type (both exact); the first term is
    ASSIGNED (not added to a zero), a row without entries is +0.  Rows of up to 32 entries are summed term by term across all rows at
    once, longer ones by np.cumsum -- a strictly sequential accumulation that starts from the first term itself."""
    T = np.dtype(dtype).type
    colptr = np.asarray(colptr, np.int64) - 1
    rows = np.asarray(rowval, np.int64) - 1
    cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
    order = np.lexsort((cols, rows))                     # by row, then by column
    rs, cs = rows[order], cols[order]
    cnt = np.bincount(rs, minlength=M)
    start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    w = (T(1) + T(0.125) * ((rs + 3 * cs) & 7).astype(dtype)).astype(dtype)
    q = T(0.25)
    short = np.nonzero(cnt <= 32)[0]
    long_rows = np.nonzero(cnt > 32)[0]
    depth = int(cnt[short].max()) if short.size else 0
    level = []                                           # level[k]: (the short rows with more than k entries, their k-th term's position)
    for k in range(depth):
        sel = short[cnt[short] > k]
        level.append((sel, start[sel] + k))

    def f(x):
        x = np.asarray(x)
        assert x.dtype == np.dtype(dtype) and x.size == N, (x.dtype, x.size)
        with np.errstate(all="ignore"):
            v = x[cs]
            t = w * (v + (q * v) * v)
            out = np.zeros(M, dtype=dtype)
            for k, (sel, at) in enumerate(level):
                out[sel] = t[at] if k == 0 else out[sel] + t[at]
            for r in long_rows:
                out[r] = np.cumsum(t[start[r]:start[r] + cnt[r]])[-1]
        return out
    return f


# ---- the complex step (src/jacobians.jl:623-648): complex arithmetic as explicit (re, im) pairs -----------------------------------------
# A complex array is a pair of real arrays of the element type.  Each function below is ONE operator of `cd` (csrc/fdjac_builtin_f.hip)
# and of fd_cplx<T> (include/fdjac_device.h), one IEEE operation per line of the device code; numpy evaluates every ufunc on its own
# (no fused multiply-add across two calls), and numpy's complex dtypes -- whose product loops may fuse and whose T(2) * z is a full
# complex product -- are not used for values.
def c_add(a, b):
    return a[0] + b[0], a[1] + b[1]


def c_sub(a, b):
    return a[0] - b[0], a[1] - b[1]


def c_mul(a, b):
    """complex * complex: (ar br - ai bi, ar bi + ai br)."""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def c_smul(s, a):
    """scalar * complex, component-wise: s * (Inf, 0) = (Inf, 0), where the full product has 0 * Inf = NaN in the imaginary part."""
    return s * a[0], s * a[1]


def c_add_s(a, s):
    return a[0] + s, a[1]


def c_sub_s(a, s):
    return a[0] - s, a[1]


def c_div_s(a, s):
    return a[0] / s, a[1] / s


def _shifted(a, fill):
    """`fill(part)` applied to both parts of a pair."""
    return fill(a[0]), fill(a[1])


def tridiag_fc(x, nl, smul=c_smul):
    """tridiag_row<cd, NL> on a pair: (xm - 2 x) + xp [+ (x x) xp]; a neighbour outside the domain is the pair (0, 0)."""
    T = x[0].dtype.type
    z = np.zeros(1, x[0].dtype)
    xm = _shifted(x, lambda p: np.concatenate([z, p[:-1]]))
    xp = _shifted(x, lambda p: np.concatenate([p[1:], z]))
    v = c_add(c_sub(xm, smul(T(2), x)), xp)
    if nl:
        v = c_add(v, c_mul(c_mul(x, x), xp))
    return v


def stencil5_fc(x, nx, ny, nl, smul=c_smul):
    """stencil5_row<cd, SK> (stencil5_pair, k_f_stencil5): (((w + e) + s) + n) - 4 c [+ (c c) e]."""
    T = x[0].dtype.type

    def nb(sl_to, sl_from):
        def fill(p):
            g = p.reshape(ny, nx)
            o = np.zeros_like(g)
            o[sl_to] = g[sl_from]
            return o
        return _shifted(x, fill)
    S = np.s_
    w, e = nb(S[:, 1:], S[:, :-1]), nb(S[:, :-1], S[:, 1:])
    s, n = nb(S[1:, :], S[:-1, :]), nb(S[:-1, :], S[1:, :])
    g = _shifted(x, lambda p: p.reshape(ny, nx))
    v = c_sub(c_add(c_add(c_add(w, e), s), n), smul(T(4), g))
    if nl:
        v = c_add(v, c_mul(c_mul(g, g), e))
    return v[0].reshape(-1), v[1].reshape(-1)


def lap7_fc(x, nx, ny, nz, smul=c_smul):
    """lap7_row<cd>: ((((((d + s) + w) + e) + n) + u) - 6 c) + (c c) e."""
    T = x[0].dtype.type

    def nb(sl_to, sl_from):
        def fill(p):
            g = p.reshape(nz, ny, nx)
            o = np.zeros_like(g)
            o[sl_to] = g[sl_from]
            return o
        return _shifted(x, fill)
    S = np.s_
    d, u = nb(S[1:], S[:-1]), nb(S[:-1], S[1:])
    s, n = nb(S[:, 1:], S[:, :-1]), nb(S[:, :-1], S[:, 1:])
    w, e = nb(S[:, :, 1:], S[:, :, :-1]), nb(S[:, :, :-1], S[:, :, 1:])
    g = _shifted(x, lambda p: p.reshape(nz, ny, nx))
    v = c_add(c_sub(c_add(c_add(c_add(c_add(c_add(d, s), w), e), n), u), smul(T(6), g)), c_mul(c_mul(g, g), e))
    return v[0].reshape(-1), v[1].reshape(-1)


def sparse_fc(M, N, colptr, rowval, dtype=F64, smul=c_smul):
    """SparseF::row<cd> on pairs: the entries (r, j) of row r in ascending j, left to right, of w * (v + (q * v) * v) -- q * v and
    w * (...) scalar * complex, (q v) * v complex * complex; the first term is ASSIGNED, a row without entries is the pair (+0, +0).
    Both parts of a long row (more than 32 entries) are accumulated strictly sequentially by np.cumsum, as in sparse_f."""
    T = np.dtype(dtype).type
    colptr = np.asarray(colptr, np.int64) - 1
    rows = np.asarray(rowval, np.int64) - 1
    cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
    order = np.lexsort((cols, rows))
    rs, cs = rows[order], cols[order]
    cnt = np.bincount(rs, minlength=M)
    start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    w = (T(1) + T(0.125) * ((rs + 3 * cs) & 7).astype(dtype)).astype(dtype)
    q = T(0.25)
    short = np.nonzero(cnt <= 32)[0]
    long_rows = np.nonzero(cnt > 32)[0]
    depth = int(cnt[short].max()) if short.size else 0
    level = [(short[cnt[short] > k], start[short[cnt[short] > k]] + k) for k in range(depth)]

    def f(x):
        assert x[0].dtype == np.dtype(dtype) and x[1].dtype == np.dtype(dtype) and x[0].size == N, (x[0].dtype, x[0].size)
        with np.errstate(all="ignore"):
            v = (x[0][cs], x[1][cs])
            t = smul(w, c_add(v, c_mul(smul(q, v), v)))
            out = (np.zeros(M, dtype=dtype), np.zeros(M, dtype=dtype))
            for k, (sel, at) in enumerate(level):
                for part in (0, 1):
                    out[part][sel] = t[part][at] if k == 0 else out[part][sel] + t[part][at]
            for r in long_rows:
                for part in (0, 1):
                    out[part][r] = np.cumsum(t[part][start[r]:start[r] + cnt[r]])[-1]
        return out
    return f


def fixture_complex(family, *prm, smul=c_smul):
    """f((re, im)) -> (re, im) of the rational built-in families on pairs of x's dtype (the parameters of `fixture`).  smul: the
    scalar * complex operator -- the CPU suite swaps in the full complex product to show that the cases tell the two apart."""
    if family == "sparse":
        M, N, colptr, rowval = prm
        fs = {}

        def f(x):
            if x[0].dtype not in fs:
                fs[x[0].dtype] = sparse_fc(M, N, colptr, rowval, x[0].dtype, smul)
            return fs[x[0].dtype](x)
        return f
    if family in ("tridiag", "tridiag_nl"):
        return lambda x: tridiag_fc(x, family == "tridiag_nl", smul)
    if family == "lap7":
        nx, ny, nz = prm
        return lambda x: lap7_fc(x, nx, ny, nz, smul)
    if family in ("lap5", "lap5_nl"):
        nx, ny = prm
        return lambda x: stencil5_fc(x, nx, ny, family == "lap5_nl", smul)
    raise ValueError(family)


def complex_epsilons(C, dtype=F64):
    """The complex step's step size: eps(T) for every colour, whatever x, relstep and absstep are (src/jacobians.jl:626)."""
    return np.full(C, np.finfo(dtype).eps, dtype=dtype)


def colour_values_complex(f_pairs, x, colors0, C, eps):
    """D[c][r] = im(f(x + i eps_c mask_c))[r] / eps_c in the element type: k_perturb MODE 2 (the pair (x_j, colour of j == c ? eps_c :
    +0)), the complex f!, entry_value<2> (the imaginary part's IEEE quotient by eps_c).  No subtraction, no f(x)."""
    x = np.asarray(x)
    T = x.dtype.type
    colors0 = np.asarray(colors0)
    D = None
    with np.errstate(all="ignore"):
        for c in range(C):
            e = T(eps[c])
            im = np.where(colors0 == c, e, T(0)).astype(x.dtype)
            _re, fi = f_pairs((x, im))
            if D is None:
                D = np.empty((C, fi.size), dtype=x.dtype)
            D[c] = fi / e
    return D if D is not None else np.empty((0, x.size), dtype=x.dtype)


def fixture(family, *prm):
    """f(x) -> f(x) in x's dtype, for the rational built-in families ("sparse", M, N, colptr, rowval: the residual of any pattern;
    "lap7", nx, ny, nz: the 7-point family)."""
    if family == "sparse":
        M, N, colptr, rowval = prm
        fs = {}

        def f(x):
            x = np.asarray(x)
            if x.dtype not in fs:
                fs[x.dtype] = sparse_f(M, N, colptr, rowval, x.dtype)
            return fs[x.dtype](x)
        return f
    if family in ("tridiag", "tridiag_nl"):
        return lambda x: tridiag_f(x, family == "tridiag_nl")
    if family == "lap7":
        nx, ny, nz = prm
        return lambda x: lap7_f(np.asarray(x), nx, ny, nz)
    if family in ("lap5", "lap5_nl"):
        nx, ny = prm
        return lambda x: stencil5_f(x, nx, ny, family == "lap5_nl")
    raise ValueError(family)


def colour_values(f, x, colors0, C, eps, fdtype, f_in=None, zero="model"):
    """D[c][r]: the value the plain evaluation stores for row r in a column of colour c; (C, M) for a residual of M rows.  f_in: the
    caller's f(x) of a forward difference -- subtracted as it is given.  zero: the form of an UNPERTURBED coordinate -- "model"
    x_i + copysign(0, eps_c) (Julia's eps * false), "library" x_i + (+0.0) whatever the sign of eps_c (k_perturb, fd_column_point: they
    differ at x_i = -0.0 for dir = -1 only, tests/test_gpu_exact_store.py), "none" x_i itself (a MUTATION: what the row-wise kernels
    once did; the CPU suites show that their cases tell it apart)."""
    x = np.asarray(x)
    T = x.dtype.type
    with np.errstate(all="ignore"):
        base = None
        if fdtype == "forward":
            base = f(x) if f_in is None else np.asarray(f_in, dtype=x.dtype)
        D = None
        for c in range(C):
            e = T(eps[c])
            z = np.copysign(T(0), e) if zero == "model" else T(0)
            m = colors0 == c
            xp = np.where(m, x + e, x if zero == "none" else x + z)
            if fdtype == "forward":
                row = (f(xp) - base) / e
            else:
                xm = np.where(m, x - e, x - z)
                row = (f(xp) - f(xm)) / (T(2) * e)
            if D is None:
                D = np.empty((C, row.size), dtype=x.dtype)
            D[c] = row
    return D if D is not None else np.empty((0, x.size), dtype=x.dtype)


def to_csc(D, colors0, colptr, rowval):
    """nzval of a 1-based CSC pattern: entry (r, j) holds D[colour of j][r], 0 for an uncoloured column."""
    colptr = np.asarray(colptr) - 1
    rows = np.asarray(rowval) - 1
    cols = np.repeat(np.arange(colptr.size - 1), np.diff(colptr))
    c = np.asarray(colors0)[cols]
    out = np.zeros(rows.size, D.dtype)
    ok = c >= 0
    out[ok] = D[c[ok], rows[ok]]
    return out


def to_dense(D, colors0, colptr, rowval, M, N):
    """The dense-J destination with a 1-based CSC sparsity pattern, column-major as an (M, N) array: entry (r, j) of the pattern holds
    D[colour of j][r]; everything else -- entries outside the pattern, the pattern's entries of a column without a colour -- holds 0
    (the reference zero-fills J before its colour loop, and so does tests/test_gpu_parity.py::test_dense_J_sparse_pattern's J)."""
    colptr = np.asarray(colptr) - 1
    rows = np.asarray(rowval) - 1
    cols = np.repeat(np.arange(N), np.diff(colptr))
    out = np.zeros((M, N), D.dtype, order="F")
    out[rows, cols] = to_csc(D, colors0, colptr + 1, rowval)
    return out


def to_banded(D, colors0, M, N, l, u):
    """BandedMatrix data, column-major (l + u + 1) x N: data[u + i - j, j] = J[i, j]; slots outside the matrix hold 0."""
    out = np.zeros((l + u + 1, N), D.dtype)
    colors0 = np.asarray(colors0)
    for b in range(l + u + 1):
        j = np.arange(N)
        i = j + b - u
        ok = (i >= 0) & (i < M) & (colors0 >= 0)
        out[b, j[ok]] = D[colors0[j[ok]], i[ok]]
    return out.T.reshape(-1)


def to_tridiagonal(D, colors0, N):
    """Tridiagonal (dl, d, du): dl[j] = J[j + 1, j], d[j] = J[j, j], du[j] = J[j, j + 1]."""
    colors0 = np.asarray(colors0)

    def take(i, j):
        out = np.zeros(i.size, D.dtype)
        ok = colors0[j] >= 0
        out[ok] = D[colors0[j[ok]], i[ok]]
        return out
    j = np.arange(N)
    return take(j[:-1] + 1, j[:-1]), take(j, j), take(j[:-1], j[:-1] + 1)


def to_banded_general(D, colors0, M, N, l, u, outside=0.0, row_shift=0):
    """to_banded with the two knobs the mutation checks turn: `outside` = what a slot of a row outside the matrix holds (the model: 0;
    NaN = "left unwritten" over a NaN-filled destination), row_shift = every slot takes the row `row_shift` below its own."""
    out = np.full((l + u + 1, N), outside, D.dtype)
    colors0 = np.asarray(colors0)
    j = np.arange(N)
    for b in range(l + u + 1):
        i = j + b - u
        inside = (i >= 0) & (i < M)
        out[b, inside & (colors0 < 0)] = 0
        ok = inside & (colors0 >= 0)
        out[b, j[ok]] = D[colors0[j[ok]], np.clip(i[ok] + row_shift, 0, M - 1)]
    return out.T.reshape(-1)


def to_blockbanded(D, colors0, layout):
    """BlockBandedMatrix data (patterns.BlockBandedLayout; ext/FiniteDiffBlockBandedMatricesExt.jl:44-68): column j of block-column J
    holds the rows of its in-band blocks K = max(J - bu, 0) .. min(J + bl, nb - 1), stacked, at block_starts(K0, J) - 1 +
    (j - off[J]) stride[J]; every one of them holds D[colour of j][row], 0 for a column without a colour."""
    colors0 = np.asarray(colors0)
    bs, nb, bl, bu = layout.blk_sizes, layout.nblk, layout.bl, layout.bu
    off = np.concatenate([[0], np.cumsum(bs)])
    out = np.zeros(layout.data_len, D.dtype)
    for J in range(nb):
        K0, K1 = max(0, J - bu), min(nb - 1, J + bl)
        r0, r1 = int(off[K0]), int(off[K1 + 1])
        st = int(layout.block_strides[J])
        s = int(layout.block_starts[(bu + K0 - J) + (bl + bu + 1) * J]) - 1
        for jj in range(int(bs[J])):
            c = int(colors0[off[J] + jj])
            if c >= 0:
                out[s + jj * st:s + jj * st + (r1 - r0)] = D[c, r0:r1]
    return out


def to_bandedblockbanded(D, colors0, layout, outside=0.0, row_shift=0):
    """BandedBlockBandedMatrix data (patterns.BandedBlockBandedLayout; ext/FiniteDiffBlockBandedMatricesExt.jl:16-42).  Every element
    of data is defined: slot t of column j (local jj, block-column J) of the slab of block (K, J) is row k = jj + t - mu of block K --
    D[colour of j][off[K] + k] where 0 <= k < n_K, an exact +0.0 where the row falls outside its block, and +0.0 in every slot of a
    column without a colour; what no slab reaches holds +0.0 (the reference zero-fills J, src/jacobians.jl:530-532).  outside /
    row_shift: the mutation knobs of to_banded_general (a slot outside its block "left unwritten"; one row off in a sub-band)."""
    colors0 = np.asarray(colors0)
    bs, nb, bl, bu, lam, mu = layout.blk_sizes, layout.nblk, layout.bl, layout.bu, layout.lam, layout.mu
    off = np.concatenate([[0], np.cumsum(bs)])
    w = bl + bu + 1
    M = int(off[-1])
    out = np.zeros(layout.data_len, D.dtype)
    for J in range(nb):
        st = int(layout.block_strides[J])
        jj = np.arange(int(bs[J]))
        c = colors0[off[J] + jj]
        for K in range(max(0, J - bu), min(nb - 1, J + bl) + 1):
            s = int(layout.block_starts[(bu + K - J) + w * J]) - 1
            for t in range(lam + mu + 1):
                k = jj + t - mu
                dest = s + jj * st + t
                inb = (k >= 0) & (k < bs[K])
                out[dest[~inb]] = outside
                out[dest[c < 0]] = 0
                ok = inb & (c >= 0)
                out[dest[ok]] = D[c[ok], np.clip(off[K] + k[ok] + row_shift, 0, M - 1)]
    return out


# ---- the rational fixtures of the structured storages (tests/jit_fixtures.py holds the functors' source) -------------------------------------
def _band_terms(N, l, u):
    i = np.arange(N)
    for d in range(-l, u + 1):
        c = i + d
        inn = (c >= 0) & (c < N)
        yield np.clip(c, 0, N - 1), inn, ((i + 3 * c) & 7)


def band_f(N, l, u, sign=False):
    """BandF (tests/jit_fixtures.py): row i = the terms of the columns c = i - l .. i + u inside the matrix, left to right, the first
    one ASSIGNED: w (v + (v / 4) v), w = 1 + ((i + 3 c) mod 8) / 8; sign=True (BandSign): ... + copysign(1, v), which sees the sign of a
    zero coordinate."""
    def f(x):
        x = np.asarray(x)
        T = x.dtype.type
        with np.errstate(all="ignore"):
            s = np.zeros(N, x.dtype)
            started = np.zeros(N, bool)
            for cc, inn, k in _band_terms(N, l, u):
                v = x[cc]
                t = (T(1) + T(0.125) * k.astype(x.dtype)) * (v + (T(0.25) * v) * v)
                if sign:
                    t = t + np.copysign(T(1), v)
                s = np.where(inn, np.where(started, s + t, t), s)
                started |= inn
        return s
    return f


def band_fc(N, l, u, smul=c_smul):
    """BandF on (re, im) pairs: w * (v + (q * v) * v) with q * v and w * (...) scalar * complex, (q v) * v complex * complex."""
    def f(x):
        T = x[0].dtype.type
        with np.errstate(all="ignore"):
            s = (np.zeros(N, x[0].dtype), np.zeros(N, x[0].dtype))
            started = np.zeros(N, bool)
            for cc, inn, k in _band_terms(N, l, u):
                v = (x[0][cc], x[1][cc])
                t = smul(T(1) + T(0.125) * k.astype(x[0].dtype), c_add(v, c_mul(smul(T(0.25), v), v)))
                a = c_add(s, t)
                s = tuple(np.where(inn, np.where(started, a[p], t[p]), s[p]) for p in (0, 1))
                started |= inn
        return s
    return f


def grid_f(nx, ny, reach):
    """GridNL (tests/jit_fixtures.py) on an nx x ny grid: s = c c; for d = 1 .. reach: s += (0.5 / d) west_d, s += ((0.25 d) east_d) c;
    s += south; s += 2 north -- a neighbour outside the grid adds the constant +0 (not a product with a zero)."""
    def f(x):
        x = np.asarray(x)
        T = x.dtype.type
        g = x.reshape(ny, nx)
        zero = np.zeros_like(g)
        with np.errstate(all="ignore"):
            s = g * g
            for d in range(1, reach + 1):
                w, e = zero.copy(), zero.copy()
                hw, he = np.zeros(g.shape, bool), np.zeros(g.shape, bool)
                if d < nx:
                    w[:, d:], hw[:, d:] = g[:, :-d], True
                    e[:, :-d], he[:, :-d] = g[:, d:], True
                s = s + np.where(hw, T(0.5 / d) * w, zero)
                s = s + np.where(he, (T(0.25 * d) * e) * g, zero)
            sv, nv = zero.copy(), zero.copy()
            hs, hn = np.zeros(g.shape, bool), np.zeros(g.shape, bool)
            sv[1:], hs[1:] = g[:-1], True
            nv[:-1], hn[:-1] = g[1:], True
            s = s + np.where(hs, sv, zero)
            s = s + np.where(hn, T(2) * nv, zero)
        return s.reshape(-1)
    return f


def _block_sums(parts, off, sign):
    """Per block and part: the block's coordinates added left to right, the first one assigned (np.cumsum: strictly sequential)."""
    out = []
    for p in parts:
        q = p + np.copysign(p.dtype.type(1), p) if sign else p
        out.append(np.array([np.cumsum(q[off[b]:off[b + 1]])[-1] for b in range(off.size - 1)], dtype=p.dtype))
    return out


def blockrat_f(blk_sizes, bl=1, bu=1, sign=False):
    """BlockRat (tests/jit_fixtures.py): row k of block b = x_k tot_b + (x_k x_k) x_k, tot_b = the sums S_J of the blocks J = b - bl ..
    b + bu inside the matrix added left to right (the first one assigned), S_J = block J's coordinates added left to right; sign=True
    (BlockSign): S_J adds v + copysign(1, v).  Any (non-empty) block sizes."""
    bs = np.asarray(blk_sizes, np.int64)
    off = np.concatenate([[0], np.cumsum(bs)])
    blk = np.repeat(np.arange(bs.size), bs)

    def f(x):
        x = np.asarray(x)
        with np.errstate(all="ignore"):
            S, = _block_sums([x], off, sign)
            tot = np.zeros(bs.size, x.dtype)
            for b in range(bs.size):
                Js = range(max(0, b - bl), min(bs.size - 1, b + bu) + 1)
                tot[b] = np.cumsum(S[list(Js)])[-1]
            return x * tot[blk] + (x * x) * x
    return f


def blockrat_fc(blk_sizes, bl=1, bu=1):
    """BlockRat on (re, im) pairs: the sums part by part, x_k * tot and (x_k * x_k) * x_k complex * complex."""
    bs = np.asarray(blk_sizes, np.int64)
    off = np.concatenate([[0], np.cumsum(bs)])
    blk = np.repeat(np.arange(bs.size), bs)

    def f(x):
        with np.errstate(all="ignore"):
            S = _block_sums(list(x), off, False)
            tot = [np.zeros(bs.size, x[0].dtype), np.zeros(bs.size, x[0].dtype)]
            for b in range(bs.size):
                Js = list(range(max(0, b - bl), min(bs.size - 1, b + bu) + 1))
                for p in (0, 1):
                    tot[p][b] = np.cumsum(S[p][Js])[-1]
            t = (tot[0][blk], tot[1][blk])
            return c_add(c_mul(x, t), c_mul(c_mul(x, x), x))
    return f


def same_bits(got, want):
    """Bit-equal, except that a NaN matches any NaN (payloads are not part of the promise)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    it = np.uint64 if got.dtype == np.float64 else np.uint32
    return (got.view(it) == want.view(it)) | (np.isnan(got) & np.isnan(want))
