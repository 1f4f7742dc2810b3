"""numpy restatement of the sparse consumer (csrc/fdjac_cscsolve.hip): the row lists, both products with their summation orders (the
long-row tree included), the order of every dot, and the whole Jacobi-preconditioned BiCGStab recurrence with its failure handling --
operation for operation, so that the device's results can be compared BIT FOR BIT.  No FMA anywhere (the library is built with
-ffp-contract=off; numpy never fuses).  Not a test file: tests/test_cscsolve_model_cpu.py and tests/test_gpu_cscsolve.py use it."""
import numpy as np

LONG = 32          # kCsLong: rows of more entries are summed by a workgroup
BLOCK = 256        # threads per workgroup
VEC_TILE = 1024    # kCsVecTile: elements per workgroup of the vector kernels


# ---- patterns (0-based colptr / rowval, int64) ----------------------------------------------------------------------------------------
def lap5_pattern(nx, ny):
    k = np.arange(nx * ny)
    i, j = k % nx, k // nx
    rows = np.stack([np.where(j > 0, k - nx, -1), np.where(i > 0, k - 1, -1), k, np.where(i < nx - 1, k + 1, -1),
                     np.where(j < ny - 1, k + nx, -1)], axis=1)
    keep = rows >= 0
    colptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return colptr, rows[keep].astype(np.int64), nx * ny


def tridiag_pattern(n):
    k = np.arange(n)
    rows = np.stack([np.where(k > 0, k - 1, -1), k, np.where(k < n - 1, k + 1, -1)], axis=1)
    keep = rows >= 0
    colptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return colptr, rows[keep].astype(np.int64), n


def random_band_pattern(n, half, per_col, seed):
    """`per_col` distinct rows per column, uniform in [j - half, j + half] (clipped); the diagonal is stored only where it is drawn."""
    rng = np.random.default_rng(seed)
    keys = rng.random((n, 2 * half + 1))
    off = np.arange(-half, half + 1)[None, :]
    rows = np.arange(n)[:, None] + off
    keys[(rows < 0) | (rows >= n)] = 2.0
    pick = np.sort(np.argpartition(keys, per_col, axis=1)[:, :per_col], axis=1)
    rv = np.take_along_axis(rows, pick, axis=1)
    colptr = (np.arange(n + 1) * per_col).astype(np.int64)
    return colptr, rv.reshape(-1).astype(np.int64), n


def odd_pattern(n, dense_row, dense_len, seed):
    """Empty rows, empty columns and one dense row of `dense_len` entries: what the long-row path and the edge cases need."""
    rng = np.random.default_rng(seed)
    cols, rows = [], []
    dense_cols = np.sort(rng.choice(n, size=dense_len, replace=False))
    for j in range(n):
        rs = set()
        if j % 7 != 3:                                   # every seventh column is empty (but for the dense row)
            for r in rng.integers(max(0, j - 40), min(n, j + 41), size=3):
                if r % 5 != 1:                           # rows r = 1 mod 5 stay empty
                    rs.add(int(r))
            if j % 3 == 0 and j % 5 != 1:
                rs.add(j)
        rs.discard(dense_row)
        rows.append(sorted(rs))
    for j in dense_cols:
        rows[j] = sorted(set(rows[j]) | {dense_row})
    colptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    rowval = np.array([r for rs in rows for r in rs], dtype=np.int64)
    return colptr, rowval, n


# ---- the row lists ------------------------------------------------------------------------------------------------------------------------
class RowLists:
    def __init__(self, colptr, rowval, N):
        colptr, rowval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64)
        self.N, self.nnz = int(N), int(rowval.size)
        self.colptr, self.rowval = colptr, rowval
        cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
        order = np.argsort(rowval, kind="stable")        # by row; within a row by slot = by column (storage order is column order)
        self.row_slot = order.astype(np.int64)
        self.row_col = cols[order]
        self.row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rowval, minlength=N))]).astype(np.int64)
        self.diag = np.full(N, -1, dtype=np.int64)
        on = np.nonzero(rowval == cols)[0]
        self.diag[cols[on]] = on
        self.lens = np.diff(self.row_ptr)
        self.nlong = int((self.lens > LONG).sum())


# ---- sums -----------------------------------------------------------------------------------------------------------------------------
def block_sum(p):
    """(..., 256) -> (...): per wavefront x += shfl_down(x, 32), 16, 8, 4, 2, 1 (lane 0), then ((w0 + w1) + w2) + w3."""
    x = p.reshape(p.shape[:-1] + (4, 64))
    for off in (32, 16, 8, 4, 2, 1):
        x = x[..., :off] + x[..., off:2 * off]
    w = x[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def strided_sum(vals):
    """Thread t of 256 adds vals[t], vals[t + 256], ... in that order, from +0.0."""
    n = vals.size
    pad = np.zeros((n + BLOCK - 1) // BLOCK * BLOCK if n else BLOCK)
    pad[:n] = vals
    acc = np.zeros(BLOCK)
    for row in pad.reshape(-1, BLOCK):
        acc = acc + row
    return acc


def _final(partials):
    return block_sum(strided_sum(partials))


def dot_vec(a, b):
    """A dot of the vector kernels: tiles of 1024, thread t adds elements t, t + 256, t + 512, t + 768, block_sum, the tiles in order."""
    prod = a * b
    nb = (prod.size + VEC_TILE - 1) // VEC_TILE
    pad = np.zeros(nb * VEC_TILE)
    pad[:prod.size] = prod
    pad = pad.reshape(nb, VEC_TILE // BLOCK, BLOCK)
    acc = np.zeros((nb, BLOCK))
    for k in range(VEC_TILE // BLOCK):
        acc = acc + pad[:, k, :]
    return _final(block_sum(acc))


def dot_rows(a, b):
    """A dot of the product kernels: tiles of 256 rows, one element per thread."""
    prod = a * b
    nb = (prod.size + BLOCK - 1) // BLOCK
    pad = np.zeros(nb * BLOCK)
    pad[:prod.size] = prod
    return _final(block_sum(pad.reshape(nb, BLOCK)))


# ---- products -------------------------------------------------------------------------------------------------------------------------
def matvec(rl, alpha, beta, nz, v, out_dtype=None):
    """y = (alpha I + beta J) v: rows of at most 32 entries left to right in ascending column, longer rows by the fixed tree."""
    out_dtype = out_dtype or v.dtype
    nz64, v64 = np.asarray(nz, dtype=np.float64), np.asarray(v, dtype=np.float64)
    prods = nz64[rl.row_slot] * v64[rl.row_col]
    acc = np.zeros(rl.N)
    short = rl.lens <= LONG
    maxlen = int(rl.lens[short].max()) if short.any() else 0
    for k in range(maxlen):
        rows = np.nonzero(short & (rl.lens > k))[0]
        acc[rows] = acc[rows] + prods[rl.row_ptr[rows] + k]
    for r in np.nonzero(~short)[0]:
        acc[r] = block_sum(strided_sum(prods[rl.row_ptr[r]:rl.row_ptr[r + 1]]))
    return (alpha * v64 + beta * acc).astype(out_dtype)


def matvec_t(rl, alpha, beta, nz, v, out_dtype=None):
    """y = (alpha I + beta J)^T v: column by column in storage order."""
    out_dtype = out_dtype or v.dtype
    nz64, v64 = np.asarray(nz, dtype=np.float64), np.asarray(v, dtype=np.float64)
    prods = nz64 * v64[rl.rowval]
    lens = np.diff(rl.colptr)
    acc = np.zeros(rl.N)
    for k in range(int(lens.max()) if lens.size else 0):
        cols = np.nonzero(lens > k)[0]
        acc[cols] = acc[cols] + prods[rl.colptr[cols] + k]
    return (alpha * v64 + beta * acc).astype(out_dtype)


# ---- BiCGStab -------------------------------------------------------------------------------------------------------------------------
def _bad(x):
    return not (abs(x) > 0.0 and abs(x) < np.inf)


def solve(rl, alpha, beta, nz, b, rtol=1e-10, max_iterations=500, keep_unconverged=False):
    """(alpha I + beta J) y = b as fd_csc_solve_async computes it.  Returns (y in b's dtype, {"flags", "iterations", "resid", "bnorm"})."""
    out_dtype = b.dtype
    with np.errstate(all="ignore"):
        nz64, b64 = np.asarray(nz, dtype=np.float64), np.asarray(b, dtype=np.float64)
        N = rl.N
        d = np.where(rl.diag >= 0, alpha + beta * nz64[np.maximum(rl.diag, 0)], np.float64(alpha)) if rl.nnz else np.full(N, np.float64(alpha))
        flags = 0
        if not np.all((np.abs(d) > 0.0) & (np.abs(d) < np.inf)):
            flags |= 2
        r, rhat = b64.copy(), b64
        p, v, y = np.zeros(N), np.zeros(N), np.zeros(N)
        bn2 = dot_vec(b64, b64)
        one = np.float64(1.0)
        rho, rho_old, al, om = bn2, one, one, one
        tol2 = (np.float64(rtol) * np.float64(rtol)) * bn2
        rn2 = bn2
        done, iters = False, 0
        if bn2 == 0.0:
            done = True
        elif flags & 2:
            done = True
        elif _bad(bn2):
            flags |= 2
            done = True
        enq = 0
        while not done and enq < max_iterations:
            enq += 1
            bk = (rho / rho_old) * (al / om)
            p = r + bk * (p - om * v)
            ph = p / d
            v = matvec(rl, alpha, beta, nz64, ph)
            rv = dot_rows(rhat, v)
            if _bad(rv):
                flags |= 2
                break
            al = rho / rv
            s = r - al * v
            sh = s / d
            sn2 = dot_vec(s, s)
            if sn2 <= tol2:                      # the first half step already meets the tolerance
                y = y + al * ph
                rn2 = sn2
                iters += 1
                done = True
                break
            t = matvec(rl, alpha, beta, nz64, sh)
            ts, tt = dot_rows(t, s), dot_rows(t, t)
            if _bad(tt):
                flags |= 2
                break
            om = ts / tt
            y = (y + al * ph) + om * sh
            r = s - om * t
            rn2, rho_new = dot_vec(r, r), dot_vec(rhat, r)
            iters += 1
            if rn2 <= tol2:
                done = True
            else:
                rho_old, rho = rho, rho_new
                if _bad(rho):
                    flags |= 2
                    break
        final = 2 if flags & 2 else (0 if done else 1)      # bit 1: breakdown; bit 0: the iterations ran out
        if final and not keep_unconverged:
            y = np.full(N, np.nan)
        return y.astype(out_dtype), {"flags": int(final), "iterations": int(iters), "resid": float(np.sqrt(rn2)), "bnorm": float(np.sqrt(bn2))}
