"""numpy restatement of the least-squares consumer (csrc/fdjac_csclsq.hip): the rectangular row lists and the long-column list, both
products with their summation orders (long rows and long columns by the fixed tree), the order of every dot, and the whole preconditioned
CGLS recurrence on the normal equations with its failure handling -- operation for operation, so that the device's results can be compared
BIT FOR BIT.  No FMA anywhere.  Not a test file: tests/test_csclsq_model_cpu.py, tests/test_gpu_csclsq.py and tests/csclsq_switch_child.py
use it."""
import numpy as np

from csc_solve_model import BLOCK, LONG, block_sum, dot_rows, dot_vec, strided_sum

DAMP_IDENTITY, DAMP_COLNORM = 0, 1


# ---- patterns with values (0-based colptr / rowval, int64) ----------------------------------------------------------------------------
def rect_band(N, half, per_col, seed, long_cols=None):
    """M = 3N/2.  Column j: the anchor rows a = floor(3j/2) and a + 1 with values 2 + u, and per_col - 2 further distinct rows
    a + U{-half..half} (clipped to the matrix) with values 0.3 u, u uniform in [-1, 1]; the columns named in `long_cols` ({column:
    length}) are padded to that length with random rows (values 0.3 u).  Returns (colptr, rowval, nzval, M, N)."""
    rng = np.random.default_rng(seed)
    M = 3 * N // 2
    long_cols = long_cols or {}
    rows, vals = [], []
    for j in range(N):
        a = 3 * j // 2
        anchors = {a, min(a + 1, M - 1)}
        rs = set(anchors)
        while len(rs) < per_col:
            rs.add(int(np.clip(a + rng.integers(-half, half + 1), 0, M - 1)))
        if j in long_cols:
            extra = rng.permutation(M)
            k = 0
            while len(rs) < long_cols[j]:
                rs.add(int(extra[k]))
                k += 1
        rs = sorted(rs)
        u = rng.uniform(-1.0, 1.0, len(rs))
        rows.append(rs)
        vals.append(np.where([r in anchors for r in rs], 2.0 + u, 0.3 * u))
    colptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return colptr, np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]), np.concatenate(vals), M, N


BAND_BIG = dict(N=20000, half=300, per_col=6, seed=3)
BAND_PADDED = dict(N=3000, half=50, per_col=5, seed=3, long_cols={100: 32, 7: 33, 1500: 300, 2999: 2500})
MU_W = ((0.0, DAMP_IDENTITY), (1e-2, DAMP_IDENTITY), (1e-2, DAMP_COLNORM), (1.0, DAMP_COLNORM))


def rect_odd(M=1500, N=2000, dense_row=77, dense_len=700, seed=1):
    """M < N, empty rows (r = 1 mod 5), empty columns (j = 3 mod 7 outside the dense row) and one dense row of `dense_len` entries.
    Returns (colptr, rowval, nzval, M, N)."""
    rng = np.random.default_rng(seed)
    dense_cols = set(np.sort(rng.choice(N, size=dense_len, replace=False)).tolist())
    rows = []
    for j in range(N):
        rs = set()
        if j % 7 != 3:
            c = j * M // N
            for r in rng.integers(max(0, c - 40), min(M, c + 41), size=3):
                if r % 5 != 1:
                    rs.add(int(r))
        rs.discard(dense_row)
        if j in dense_cols and j % 7 != 3:
            rs.add(dense_row)
        rows.append(sorted(rs))
    colptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    rowval = np.array([r for rs in rows for r in rs], dtype=np.int64)
    nz = rng.uniform(-1.0, 1.0, rowval.size)
    return colptr, rowval, nz, M, N


# ---- the lists ------------------------------------------------------------------------------------------------------------------------
class RectLists:
    """The pattern by rows (a stable counting sort of the entries by row: within a row by slot = by column), the rows and the columns
    of more than LONG entries (the columns in ascending order)."""

    def __init__(self, colptr, rowval, M, N):
        colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
        self.M, self.N, self.nnz = int(M), int(N), int(rowval.size)
        self.colptr, self.rowval = colptr, rowval
        cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
        order = np.argsort(rowval, kind="stable")
        self.row_slot = order.astype(np.int64)
        self.row_col = cols[order]
        self.row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rowval, minlength=M))]).astype(np.int64)
        self.lens = np.diff(self.row_ptr)
        self.nlong = int((self.lens > LONG).sum())
        self.col_lens = np.diff(colptr)
        self.long_cols = np.nonzero(self.col_lens > LONG)[0].astype(np.int64)


# ---- products -------------------------------------------------------------------------------------------------------------------------
def _segment_sums(ptr, lens, prods, n):
    """Segments of at most LONG terms left to right from +0.0; longer ones: thread t adds terms t, t + 256, ..., then block_sum."""
    acc = np.zeros(n)
    short = lens <= LONG
    maxlen = int(lens[short].max()) if short.any() else 0
    for k in range(maxlen):
        seg = np.nonzero(short & (lens > k))[0]
        acc[seg] = acc[seg] + prods[ptr[seg] + k]
    for i in np.nonzero(~short)[0]:
        acc[i] = block_sum(strided_sum(prods[ptr[i]:ptr[i + 1]]))
    return acc


def rows_product(rl, nz64, v64):
    """J v in Float64: every row in ascending column."""
    return _segment_sums(rl.row_ptr, rl.lens, nz64[rl.row_slot] * v64[rl.row_col], rl.M)


def cols_product(rl, nz64, v64):
    """J^T v in Float64: every column in storage order."""
    return _segment_sums(rl.colptr, rl.col_lens, nz64 * v64[rl.rowval], rl.N)


def col_norms(rl, nz64):
    """g_j = sum_i J_ij^2 in the columns' order."""
    return _segment_sums(rl.colptr, rl.col_lens, nz64 * nz64, rl.N)


def matvec(rl, nz, v, transpose=False):
    """fd_csc_lsq_matvec_async: y = J v or J^T v in v's dtype."""
    nz64, v64 = np.asarray(nz, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return (cols_product if transpose else rows_product)(rl, nz64, v64).astype(v.dtype)


# ---- preconditioned CGLS ----------------------------------------------------------------------------------------------------------------
def _bad(x):
    return not (abs(x) > 0.0 and abs(x) < np.inf)


def _not_finite(x):
    return not (abs(x) < np.inf)


def solve(rl, mu, kind, nz, b, rtol=1e-10, max_iterations=500, keep_unconverged=False):
    """(J^T J + mu W) y = J^T b as fd_csc_lsq_solve_async computes it.  Returns (y, r_out, status): y and r_out in b's dtype,
    status = {"flags", "iterations", "grad", "grad0"}."""
    out_dtype = b.dtype
    with np.errstate(all="ignore"):
        nz64 = np.asarray(nz, dtype=np.float64)
        mu = np.float64(mu)
        N = rl.N
        r = np.asarray(b, dtype=np.float64).copy()
        y = np.zeros(N)
        g = col_norms(rl, nz64)
        s = cols_product(rl, nz64, r)
        w = g if kind == DAMP_COLNORM else np.ones(N)
        m = g + mu * w
        flags = 0
        if not np.all((np.abs(m) > 0.0) & (np.abs(m) < np.inf)):
            flags |= 2
        z = s / m
        p = z.copy()
        gamma, gn2, pi = dot_rows(s, z), dot_rows(s, s), dot_rows(w * z, z)
        g02 = gn2
        tol2 = (np.float64(rtol) * np.float64(rtol)) * gn2
        done, iters = False, 0
        if gn2 == 0.0:
            done = True
        elif flags & 2:
            done = True
        elif _not_finite(gamma):
            flags |= 2
            done = True
        enq = 0
        while not done and enq < max_iterations:
            enq += 1
            q = rows_product(rl, nz64, p)
            delta = dot_rows(q, q) + mu * pi
            if _bad(delta):
                flags |= 2
                break
            alpha = gamma / delta
            r = r - alpha * q
            y = y + alpha * p
            s = cols_product(rl, nz64, r) - mu * (w * y)
            z = s / m
            gamma_new, gn2 = dot_rows(s, z), dot_rows(s, s)
            iters += 1
            if gn2 <= tol2:
                done = True
                break
            if _not_finite(gamma_new):
                flags |= 2
                break
            beta = gamma_new / gamma
            gamma = gamma_new
            p = z + beta * p
            pi = dot_vec(w * p, p)
        final = 2 if flags & 2 else (0 if done else 1)      # bit 1: breakdown; bit 0: the iterations ran out
        if final and not keep_unconverged:
            y, r = np.full(N, np.nan), np.full(rl.M, np.nan)
        return (y.astype(out_dtype), r.astype(out_dtype),
                {"flags": int(final), "iterations": int(iters), "grad": float(np.sqrt(gn2)), "grad0": float(np.sqrt(g02))})
