"""numpy model of the pivoted tridiagonal solve (csrc/fdjac_solve.hip, the k_tripiv_* kernels; DESIGN §4.4 "Pivoted solve"): a recursive
partitioned solve with partial pivoting inside every partition.  Every operation is a Float64 numpy ufunc in the order the kernels use
(no fused multiply-add, IEEE division), so the device's y and status word must EQUAL what this returns, bit for bit.

Vectorised over the chunks of a level, scalar in the elimination step.  Nothing here runs on the GPU.

  step      two rows with the same leading interior unknown x_j: the accumulated row (f, p, q, 0, s) on (x_first, x_j, x_j+1) and the
            matrix row (0, a, b, c, d) on (x_j, x_j+1, x_j+2).  The pivot is the accumulated row if |p| >= |a| (a tie keeps it), else
            the matrix row; l = other.lead / pivot.lead; new accumulated row = other - l * pivot (the products l * 0 are formed).
  chunk     8 consecutive rows of a level.  The downward sweep starts from row 1 and steps with rows 2 .. 7: E_B on (x_0, x_7, x_8); the
            upward sweep starts from row 6 and steps with rows 5 .. 0, a and c exchanged: E_A on (x_-1, x_0, x_7).  The coarse level has
            the unknowns (x_0, x_7) of every chunk, rows E_A, E_B.  The last chunk has its true length m: the same sweeps over m >= 3
            rows; m = 2, 1: its rows are its coarse rows.
  bottom    a level of at most 8 rows: the accumulated row starts as row 0 with f = 0 and steps with rows 1 .. n - 1 (dgtsv's
            elimination), then back-substitutes.
  substitution  x_0, x_7 of a chunk and x_8 (0 past the end) come from the coarse level; the downward sweep is repeated and, for
            j = 6 .. 1, x_j = (rhs - f * x_0 - n1 * x_j+1 - n2 * x_j+2) / lead over the pivot row kept for x_j, left to right.

Status: bit 0 = a level-0 row is not diagonally dominant (reported, never a refusal); bit 2 (value 4) = a pivot lead was 0 or not
finite, y is then all NaN."""
from collections import namedtuple

import numpy as np

KCHUNK = 8            # fdjac_solve.hip: kChunk
KPIVTOP = 2048        # fdjac_solve.hip: kPivTop, a level of at most this many rows is finished inside one workgroup
NOT_DOMINANT, BAD_PIVOT = 1, 4

PivResult = namedtuple("PivResult", "y status swaps")
#   swaps: per level of the recursion (level 0 first, the bottom solve last) one bool array of every pivot choice of that level's
#   reduction (True = the matrix row was the pivot); the bottom solve's choices are the last entry


def next_rows(n):
    nc = -(-n // KCHUNK)
    m = n - KCHUNK * (nc - 1)
    return 2 * (nc - 1) + min(m, 2)


def piv_levels(N):
    """Rows of every level that has a launch of its own: N, ..., the top (<= 2048 rows, one workgroup)."""
    ns = [int(N)]
    while ns[-1] > KPIVTOP:
        ns.append(next_rows(ns[-1]))
    return ns


def piv_all_levels(N):
    """Rows of every level of the recursion, down to the one of at most 8 rows that one thread solves."""
    ns = [int(N)]
    while ns[-1] > KCHUNK:
        ns.append(next_rows(ns[-1]))
    return ns


def step(acc, mat):
    """One elimination step (see above), elementwise over arrays.  -> new accumulated row (f, p, q, s), the pivot row
    (f, lead, n1, n2, rhs), the choice and whether the pivot's lead was 0 or not finite."""
    f, p, q, s = acc
    a, b, c, d = mat
    zero = np.zeros_like(p)
    swap = ~(np.abs(p) >= np.abs(a))
    pf, pl, pn1, pn2, pr = np.where(swap, zero, f), np.where(swap, a, p), np.where(swap, b, q), np.where(swap, c, zero), np.where(swap, d, s)
    of, ol, on1, on2, orh = np.where(swap, f, zero), np.where(swap, p, a), np.where(swap, q, b), np.where(swap, zero, c), np.where(swap, s, d)
    l = ol / pl
    new = (of - l * pf, on1 - l * pn1, on2 - l * pn2, orh - l * pr)
    bad = ~(np.isfinite(pl) & (pl != 0.0))
    return new, (pf, pl, pn1, pn2, pr), swap, bad


def _down(a, b, c, d):
    """Downward sweep over chunks of m >= 3 rows (arrays of shape (chunks, m)) -> E_B = (f, p, q, s), pivot rows of x_1 .. x_m-2."""
    m = a.shape[1]
    acc = (a[:, 1], b[:, 1], c[:, 1], d[:, 1])
    pivs, swaps, bad = [], [], np.zeros(a.shape[0], bool)
    for j in range(2, m):
        acc, piv, sw, bd = step(acc, (a[:, j], b[:, j], c[:, j], d[:, j]))
        pivs.append(piv); swaps.append(sw); bad |= bd
    return acc, pivs, swaps, bad


def _up(a, b, c, d):
    """Upward sweep: the mirror image, a and c exchanged -> E_A = (f, p, q, s) on (x_m-1, x_0, x_-1)."""
    m = a.shape[1]
    acc = (c[:, m - 2], b[:, m - 2], a[:, m - 2], d[:, m - 2])
    swaps, bad = [], np.zeros(a.shape[0], bool)
    for j in range(m - 3, -1, -1):
        acc, _piv, sw, bd = step(acc, (c[:, j], b[:, j], a[:, j], d[:, j]))
        swaps.append(sw); bad |= bd
    return acc, swaps, bad


def _split(n):
    """(full chunks, rows of the last chunk if it is not full else 0)."""
    nc = -(-n // KCHUNK)
    m = n - KCHUNK * (nc - 1)
    return (nc, 0) if m == KCHUNK else (nc - 1, m)


def reduce_level(rows):
    """rows = (a, b, c, d) of n > 8 rows -> the coarse level's rows, the pivot choices, whether a pivot was bad."""
    a, b, c, d = rows
    n = a.size
    F, m = _split(n)
    out = [np.zeros(next_rows(n)) for _ in range(4)]
    swaps, bad = [], False
    if F:
        blk = [v[:KCHUNK * F].reshape(F, KCHUNK) for v in rows]
        eb, _p, sd, bd = _down(*blk)
        ea, su, bu = _up(*blk)
        # E_A on (x_-1, x_0, x_7): a = q, b = p, c = f;  E_B on (x_0, x_7, x_8): a = f, b = p, c = q
        for o, va, vb in zip(out, (ea[2], ea[1], ea[0], ea[3]), (eb[0], eb[1], eb[2], eb[3])):
            o[0:2 * F:2] = va
            o[1:2 * F:2] = vb
        swaps += sd + su
        bad = bool(np.any(bd | bu))
    if m >= 3:
        blk = [v[KCHUNK * F:].reshape(1, m) for v in rows]
        eb, _p, sd, bd = _down(*blk)
        ea, su, bu = _up(*blk)
        for o, va, vb in zip(out, (ea[2], ea[1], ea[0], ea[3]), (eb[0], eb[1], eb[2], eb[3])):
            o[2 * F] = va[0]
            o[2 * F + 1] = vb[0]
        swaps += sd + su
        bad = bad or bool(np.any(bd | bu))
    elif m:
        for o, v in zip(out, rows):
            o[2 * F:] = v[KCHUNK * F:]
    return tuple(out), (np.concatenate(swaps) if swaps else np.zeros(0, bool)), bad


def _backsub(pivs, x0, xlast, xnext, m):
    """x_1 .. x_m-2 of chunks of m rows from the pivot rows of the downward sweep."""
    x = [None] * (m + 1)
    x[0], x[m - 1], x[m] = x0, xlast, xnext
    for j in range(m - 2, 0, -1):
        f, lead, n1, n2, rhs = pivs[j - 1]
        x[j] = (rhs - f * x0 - n1 * x[j + 1] - n2 * x[j + 2]) / lead
    return x[:m]


def substitute_level(rows, X):
    """The solution of a level of n > 8 rows from the solved coarse level X."""
    n = rows[0].size
    F, m = _split(n)
    x = np.zeros(n)
    Xp = np.concatenate([X, [0.0]])
    if F:
        blk = [v[:KCHUNK * F].reshape(F, KCHUNK) for v in rows]
        _eb, pivs, _s, _b = _down(*blk)
        k = np.arange(F)
        cols = _backsub(pivs, Xp[2 * k], Xp[2 * k + 1], Xp[2 * k + 2], KCHUNK)
        x[:KCHUNK * F] = np.stack(cols, axis=1).reshape(-1)
    if m >= 3:
        blk = [v[KCHUNK * F:].reshape(1, m) for v in rows]
        _eb, pivs, _s, _b = _down(*blk)
        cols = _backsub(pivs, Xp[2 * F:2 * F + 1], Xp[2 * F + 1:2 * F + 2], np.zeros(1), m)
        x[KCHUNK * F:] = np.stack(cols, axis=1).reshape(-1)
    elif m:
        x[KCHUNK * F:] = X[2 * F:]
    return x


def solve_bottom(rows):
    """A level of n <= 8 rows, one thread: dgtsv's elimination by the same step, then back-substitution."""
    a, b, c, d = [v.reshape(1, -1) for v in rows]
    n = a.shape[1]
    zero = np.zeros(1)
    acc = (zero, b[:, 0], c[:, 0], d[:, 0])
    pivs, swaps, bad = [], [], False
    for j in range(1, n):
        acc, piv, sw, bd = step(acc, (a[:, j], b[:, j], c[:, j], d[:, j]))
        pivs.append(piv); swaps.append(sw); bad = bad or bool(bd[0])
    pivs.append((acc[0], acc[1], acc[2], zero, acc[3]))       # the pivot row of x_n-1
    bad = bad or not (np.isfinite(acc[1][0]) and acc[1][0] != 0.0)
    x = [None] * n + [zero, zero]
    for j in range(n - 1, -1, -1):
        f, lead, n1, n2, rhs = pivs[j]
        x[j] = (rhs - f * zero - n1 * x[j + 1] - n2 * x[j + 2]) / lead
    return np.concatenate(x[:n]), (np.concatenate(swaps) if swaps else np.zeros(0, bool)), bad


def level0_rows(dl, d, du, rhs, alpha, beta, layout="diagonals"):
    """a, b, c, d of alpha I + beta J as the level-0 loaders form them (Float64 arithmetic on the stored values).  The coefficient that
    does not exist (a of the first row, c of the last) is 0.0 on the diagonals layout and beta * 0.0 on the CSC layout."""
    N = np.asarray(d).size
    alpha, beta = np.float64(alpha), np.float64(beta)
    none = np.float64(0.0) if layout == "diagonals" else beta * np.float64(0.0)
    a = np.full(N, none)
    c = np.full(N, none)
    a[1:] = beta * np.asarray(dl, dtype=np.float64)
    c[:-1] = beta * np.asarray(du, dtype=np.float64)
    b = alpha + beta * np.asarray(d, dtype=np.float64)
    return a, b, c, np.asarray(rhs, dtype=np.float64).copy()


def piv_solve_rows(rows, dtype=np.float64):
    """The solve of the system whose level-0 rows are (a, b, c, d) -> PivResult."""
    with np.errstate(all="ignore"):
        a, b, c, _d = rows
        status = NOT_DOMINANT if bool(np.any(~(np.abs(b) >= np.abs(a) + np.abs(c)))) else 0
        levels, swaps, bad = [tuple(rows)], [], False
        while levels[-1][0].size > KCHUNK:
            nxt, sw, bd = reduce_level(levels[-1])
            levels.append(nxt); swaps.append(sw); bad = bad or bd
        x, sw, bd = solve_bottom(levels[-1])
        swaps.append(sw); bad = bad or bd
        for lv in reversed(levels[:-1]):
            x = substitute_level(lv, x)
        if bad:
            status |= BAD_PIVOT
            x = np.full(x.size, np.nan)
        return PivResult(x.astype(dtype), status, swaps)


def piv_solve(dl, d, du, rhs, alpha=0.0, beta=1.0, layout="diagonals", dtype=np.float64):
    """(alpha I + beta J) y = rhs for J = Tridiagonal(dl, d, du) in the solver's element type `dtype`."""
    dl, d, du, rhs = [np.asarray(v, dtype=dtype) for v in (dl, d, du, rhs)]
    return piv_solve_rows(level0_rows(dl, d, du, rhs, alpha, beta, layout), dtype)


# ---------------------------------------------------------------------------------------------------------------- inputs
FAMILIES = ("advect", "zero_diag", "gauss", "osc")
SIZES = [1, 2, 3, 8, 9, 10, 11, 16, 17, 2048, 2049, 2050, 2057, 16385, 16386, 70001]


def family(name, N, seed=0, dtype=np.float64):
    """(dl, d, du, rhs) of J for one of the four families (a_0 = c_N-1 = 0 by construction), in `dtype`."""
    rng = np.random.default_rng([seed, N, FAMILIES.index(name)])
    if name == "advect":
        dl, d, du = np.full(N - 1, -3.0), np.full(N, 1.0), np.full(N - 1, 3.0)
    elif name == "zero_diag":
        dl, d, du = np.full(N - 1, 1.0), np.zeros(N), np.full(N - 1, 1.0)
    elif name == "gauss":
        dl, d, du = rng.standard_normal(N - 1), rng.standard_normal(N), rng.standard_normal(N - 1)
    elif name == "osc":
        dl, d, du = np.full(N - 1, 1.0), np.full(N, 2.0 * np.cos(0.7)), np.full(N - 1, 1.0)
    else:
        raise ValueError(name)
    rhs = rng.standard_normal(N)
    return tuple(np.asarray(v, dtype=dtype) for v in (dl, d, du, rhs))


def family_sizes(name):
    return [N for N in SIZES if not (name == "zero_diag" and N % 2)]


def system_of(dl, d, du, rhs, alpha, beta):
    """tests/solve_model.py's System of the matrix the device sees (for refined_reference)."""
    from solve_model import System
    a, b, c, r = level0_rows(dl, d, du, rhs, alpha, beta)
    N = b.size
    A = {-1: a + 0.0, 0: b, 1: c + 0.0} if N > 1 else {0: b}
    return System("tri", N, alpha, beta, (dl, d, du), r, A, None, {})


# ---------------------------------------------------------------------------------------------------------------- the accuracy bound
# ||y - y_ref||_inf <= F * max(E_lapack, eps * ||y_ref||_inf) against SciPy's pivoted banded LU refined in extended precision;
# F = 4 x the model's worst ratio of the family over SIZES (profiles/solver_accuracy_pivot.md; the margin because other seeds move the
# ratio by small factors), capped at 1024
EPS = np.finfo(np.float64).eps
MEASURED = {"advect": 1.07, "zero_diag": 0.559, "gauss": 5.68, "osc": 24.1}      # worst ratio per family, rounded up
F_CAP = 1024.0


def bound_factor(name):
    return min(4.0 * MEASURED[name], F_CAP)


def degenerate_11():
    """N = 11 = a chunk of 8 and one of 3 whose two sweeps both start from row 9; with b_9 = 0 both pivot on their other row with
    l = 0 and return row 9 itself: E_A = E_B, the coarse system is singular although the matrix is not."""
    N = 11
    d = np.full(N, 2.0)
    d[9] = 0.0
    return np.ones(N - 1), d, np.ones(N - 1), np.arange(1.0, N + 1)
