"""Host model of the device column colouring (fd_color_columns_device, csrc/fdjac_color.hip): pure numpy, no library.

The contract (include/fdjac.h): the column intersection graph of a CSC pattern -- two columns conflict when they share a row -- is
coloured greedily in order of DESCENDING priority, prio(j) = murmur3's 64-bit finaliser of j + 0x9E3779B97F4A7C15 (mod 2^64), a
bijection (no ties).  A column takes the smallest colour (1-based) that none of its conflicting columns of higher priority uses; a
column without entries conflicts with nothing and gets colour 1.  Jones-Plassmann on the device produces exactly this vector, whatever
its schedule; tests/test_gpu_color.py compares element for element.

`colptr` / `rowval` are `base`-based integer arrays (the tests use the reference's 1-based ones).
"""
import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xFF51AFD7ED558CCD)
_M2 = np.uint64(0xC4CEB9FE1A85EC53)
_S = np.uint64(33)


def prio(j):
    """The priority of column(s) j (0-based), uint64 arithmetic modulo 2^64."""
    with np.errstate(over="ignore"):
        x = np.asarray(j).astype(np.uint64) + _GOLDEN
        x ^= x >> _S
        x *= _M1
        x ^= x >> _S
        x *= _M2
        x ^= x >> _S
    return x


def _transpose(M, colptr, rowval, base):
    """Row lists of the pattern: (row_ptr[M + 1], row_cols[nnz]) with 0-based columns."""
    colptr = np.asarray(colptr, np.int64) - base
    rows = np.asarray(rowval, np.int64)[colptr[0]:colptr[-1]] - base
    cols = np.repeat(np.arange(colptr.size - 1, dtype=np.int64), np.diff(colptr))
    order = np.argsort(rows, kind="stable")
    row_ptr = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=M), out=row_ptr[1:])
    return colptr, rows, row_ptr, cols[order]


def conflicts(M, N, colptr, rowval, base=1):
    """For every column the sorted array of the OTHER columns it shares a row with."""
    colptr, rows, row_ptr, row_cols = _transpose(M, colptr, rowval, base)
    out = []
    for j in range(N):
        rs = rows[colptr[j] - colptr[0]:colptr[j + 1] - colptr[0]]
        if rs.size == 0:
            out.append(np.empty(0, np.int64))
            continue
        nb = np.unique(np.concatenate([row_cols[row_ptr[r]:row_ptr[r + 1]] for r in rs]))
        out.append(nb[nb != j])
    return out


def max_conflicts(M, N, colptr, rowval, base=1):
    """Delta: the largest number of conflicting columns of any column (greedy uses at most Delta + 1 colours)."""
    return max((c.size for c in conflicts(M, N, colptr, rowval, base)), default=0)


def greedy(M, N, colptr, rowval, base=1):
    """The colour vector (int64, 1-based colours) of the contract: sequential greedy in order of descending priority."""
    nbrs = conflicts(M, N, colptr, rowval, base)
    p = prio(np.arange(N))
    colors = np.zeros(N, np.int64)
    for j in np.argsort(p)[::-1]:
        used = colors[nbrs[j]]                 # 0 = not coloured yet = lower priority: forbids nothing
        used = np.unique(used[used > 0])
        # the smallest positive integer not in `used` (sorted, distinct): the first index where used[i] != i + 1
        gap = np.nonzero(used != np.arange(1, used.size + 1))[0]
        colors[j] = (gap[0] if gap.size else used.size) + 1
    return colors


def valid(M, colptr, rowval, colors, base=1):
    """True iff no row holds two columns of the same non-zero colour."""
    return bad_rows(M, colptr, rowval, colors, base) == 0


def bad_rows(M, colptr, rowval, colors, base=1):
    """The number of rows in which two columns of the same non-zero colour meet (fd_color_check_device)."""
    _colptr, _rows, row_ptr, row_cols = _transpose(M, colptr, rowval, base)
    c = np.asarray(colors, np.int64)[row_cols]
    r = np.repeat(np.arange(M, dtype=np.int64), np.diff(row_ptr))
    r, c = r[c > 0], c[c > 0]
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    dup = (r[1:] == r[:-1]) & (c[1:] == c[:-1])
    return int(np.unique(r[1:][dup]).size)


# ---- the patterns the colouring tests share (1-based colptr / rowval, int64) ------------------------------------------------------------
def random_band(M, N, per_col, reach, seed, empty=0.03):
    """The generator of tests/test_gpu_jit.py (`_random_band`): `per_col` rows within +-`reach` of the column's centre, duplicates
    dropped, a fraction `empty` of the columns without entries."""
    rng = np.random.default_rng(seed)
    centre = (np.arange(N) * M) // max(N, 1)
    offs = np.sort(rng.integers(-reach, reach + 1, size=(N, per_col)), axis=1)
    rows = centre[:, None] + offs
    keep = (rows >= 0) & (rows < M)
    keep[:, 1:] &= rows[:, 1:] != rows[:, :-1]
    keep[rng.random(N) < empty] = False
    colptr = np.empty(N + 1, np.int64)
    colptr[0] = 1
    np.cumsum(keep.sum(axis=1), out=colptr[1:])
    colptr[1:] += 1
    return colptr, (rows[keep] + 1).astype(np.int64)


def dense_row(M, N, seed=0):
    """Row 0 holds every column (a clique: N colours, N levels); every column has one more entry in a random other row."""
    other = np.random.default_rng(seed).integers(1, M, size=N)
    colptr = 1 + 2 * np.arange(N + 1, dtype=np.int64)
    rowval = np.stack([np.ones(N, np.int64), other.astype(np.int64) + 1], axis=1).reshape(-1)
    return colptr, rowval


def random_40x60():
    """The random rectangular pattern of tests/test_abi_cpu.py::test_matrix_colors_plan_time_colouring, as a boolean matrix."""
    return np.random.default_rng(0).random((40, 60)) < 0.08
