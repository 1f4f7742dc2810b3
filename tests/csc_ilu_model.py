"""numpy restatement of the block ILU(0) preconditioner of the sparse consumer (csrc/fdjac_cscsolve.hip: k_cs_ilu_factor,
k_cs_ilu_apply and the PC = 1 instances of the vector kernels): the schedule, the factorisation and the triangular solves, operation for
operation, and the BiCGStab recurrence around them with the dots and products of tests/csc_solve_model.py -- so that the device's
levels, factors, y, iteration count, residual norm and flags can be compared BIT FOR BIT.  Not a test file:
tests/test_cscilu_model_cpu.py and tests/test_gpu_cscilu.py use it.

Definitions.
  Blocks: the uniform contiguous ranges [k bs, min((k + 1) bs, N)), bs in 2..1024; the last block may be shorter.
  In-block entry: a stored entry whose row and column lie in the same block (a contiguous run of the row's sorted list).
  The matrix: A = alpha I + beta J.  An off-diagonal stored entry is beta * nzval (one multiply, no addition); the diagonal is
  alpha + beta * nzval, or alpha where it is not stored.  The diagonal is always part of the factor's pattern; it lives in u (N doubles).
  All arithmetic is Float64 for either element type; nothing is contracted into an FMA (numpy never fuses).

Factorisation, once per solve: every block by IKJ ILU(0).  Row i: form the in-block values w_j and d_i as above.  For every in-block
(i, k), k < i, in ascending k: l = w_k / u_k; w_k = l; for every in-block (k, j) of row k with j > k, in ascending j, f its final value:
j == i: d_i = d_i - l * f; otherwise, if (i, j) is stored in-block: w_j = w_j - l * f (one multiply, one subtraction; an entry that
is not stored is dropped).  Then u_i = d_i.  A u_i that is zero or not finite is a breakdown (the solve ends with flags 2 and no
iteration); the arithmetic goes on regardless.
The factor: lu, nnz doubles indexed like the row lists -- l_ik at the in-block lower positions, the final upper values at the in-block
upper positions, u_i at a stored diagonal's position, +0.0 at every position outside the block -- and u, N doubles.

Apply, z = M^-1 x per block.  Forward, i ascending: t = x_i; for the in-block lower entries in ascending k: t = t - l_ik * z_k; z_i = t.
Backward, i descending: t = z_i; for the in-block upper entries in ascending j: t = t - u_ij * z_j; z_i = t / u_i (an IEEE division).

Schedule: lev_f(i) = 0 if row i has no in-block lower entry, else 1 + max lev_f(k) over those entries; lev_b(i) likewise over the
in-block upper entries.  Per block the rows are ordered by (level, row).  A row reads only rows of lower levels, so the device's
level-by-level order gives the bits of the row order: factor(order="level") shows it."""
import numpy as np

import csc_solve_model as M

BS_MAX = 1024


class Schedule:
    """The runs and the levels of the pattern `rl` (csc_solve_model.RowLists) for blocks of bs rows.  lo / mid / up / hi: per row the
    positions in the row lists of the first in-block entry, the first with column >= row, the first with column > row, the run's end."""

    def __init__(self, rl, bs):
        assert 2 <= int(bs) <= BS_MAX
        N = rl.N
        self.rl, self.bs, self.N = rl, int(bs), N
        i = np.arange(N, dtype=np.int64)
        b0 = i // bs * bs
        b1 = np.minimum(b0 + bs, N)
        key = np.repeat(i, rl.lens) * (N + 1) + rl.row_col        # ascending: rows ascend, and the columns within a row
        self.lo = np.searchsorted(key, i * (N + 1) + b0)
        self.mid = np.searchsorted(key, i * (N + 1) + i)
        self.up = np.searchsorted(key, i * (N + 1) + i + 1)
        self.hi = np.searchsorted(key, i * (N + 1) + b1)
        col = rl.row_col
        self.lev_f = np.zeros(N, dtype=np.int32)
        self.lev_b = np.zeros(N, dtype=np.int32)
        for r in range(N):
            if self.mid[r] > self.lo[r]:
                self.lev_f[r] = 1 + self.lev_f[col[self.lo[r]:self.mid[r]]].max()
        for r in range(N - 1, -1, -1):
            if self.hi[r] > self.up[r]:
                self.lev_b[r] = 1 + self.lev_b[col[self.up[r]:self.hi[r]]].max()
        # the vectorised apply: per level (all blocks at once: a row reads its own block only) the rows, ascending
        self.rows_f = [np.nonzero(self.lev_f == L)[0] for L in range(int(self.lev_f.max()) + 1 if N else 0)]
        self.rows_b = [np.nonzero(self.lev_b == L)[0] for L in range(int(self.lev_b.max()) + 1 if N else 0)]

    def level_order(self):
        """The rows in the order the device's lanes are numbered: block by block, by (forward level, row)."""
        i = np.arange(self.N)
        return np.lexsort((i, self.lev_f, i // self.bs))


def levels(rl, bs):
    """-> (lev_f, lev_b), Int32 (N,)."""
    s = Schedule(rl, bs)
    return s.lev_f, s.lev_b


def _bad(x):
    return not (abs(x) > 0.0 and abs(x) < np.inf)


def factor(sch, alpha, beta, nz, order="row"):
    """-> (lu (nnz,), u (N,), bad).  order = "row": rows ascending; "level": block by block, by (forward level, row), as the device
    schedules them -- the same bits."""
    rl, N = sch.rl, sch.N
    col, slot = rl.row_col, rl.row_slot
    nz64 = np.asarray(nz, dtype=np.float64)
    alpha, beta = np.float64(alpha), np.float64(beta)
    lu, u = np.zeros(rl.nnz), np.full(N, np.nan)
    bad = False
    rows = range(N) if order == "row" else sch.level_order()
    assert order in ("row", "level")
    with np.errstate(all="ignore"):
        for i in rows:
            lo, mid, up, hi = int(sch.lo[i]), int(sch.mid[i]), int(sch.up[i]), int(sch.hi[i])
            w = beta * nz64[slot[lo:hi]]                              # the run's values; the diagonal's (if stored) is replaced by d below
            d = alpha + w[mid - lo] if up > mid else alpha
            pos = {int(c): p for p, c in enumerate(col[lo:hi])}
            for p in range(lo, mid):
                k = int(col[p])
                l = w[p - lo] / u[k]
                w[p - lo] = l
                for q in range(int(sch.up[k]), int(sch.hi[k])):
                    j, f = int(col[q]), lu[q]
                    if j == i:
                        d = d - l * f
                    elif j in pos:
                        w[pos[j]] = w[pos[j]] - l * f
            if up > mid:
                w[mid - lo] = d
            lu[lo:hi] = w
            u[i] = d
            bad = bad or _bad(d)
    return lu, u, bad


def apply(sch, lu, u, x):
    """z = (L U)^-1 x per block: the forward levels ascending, then the backward levels; within a row the entries in ascending column."""
    col = sch.rl.row_col
    z = np.array(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        for rows in sch.rows_f[1:]:
            a, n = sch.lo[rows], sch.mid[rows] - sch.lo[rows]
            t = z[rows]
            for k in range(int(n.max())):
                on = n > k
                t[on] = t[on] - lu[a[on] + k] * z[col[a[on] + k]]
            z[rows] = t
        for rows in sch.rows_b:
            a, n = sch.up[rows], sch.hi[rows] - sch.up[rows]
            t = z[rows]
            for k in range(int(n.max()) if rows.size else 0):
                on = n > k
                t[on] = t[on] - lu[a[on] + k] * z[col[a[on] + k]]
            z[rows] = t / u[rows]
    return z


def apply_by_rows(sch, lu, u, x):
    """The apply as the definition states it, row by row (the tests compare it with the level-wise one above)."""
    col = sch.rl.row_col
    z = np.array(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(sch.N):
            t = z[i]
            for p in range(int(sch.lo[i]), int(sch.mid[i])):
                t = t - lu[p] * z[col[p]]
            z[i] = t
        for i in range(sch.N - 1, -1, -1):
            t = z[i]
            for p in range(int(sch.up[i]), int(sch.hi[i])):
                t = t - lu[p] * z[col[p]]
            z[i] = t / u[i]
    return z


def solve(rl, alpha, beta, nz, b, rtol=1e-10, max_iterations=500, keep_unconverged=False, bs=256, sch=None):
    """(alpha I + beta J) y = b as fd_csc_solve_async computes it after fd_csc_solver_set_block_ilu(solver, bs): the recurrence of
    csc_block_model.solve with the apply exchanged.  Returns (y in b's dtype, {"flags", "iterations", "resid", "bnorm"})."""
    sch = sch or Schedule(rl, bs)
    assert sch.bs == int(bs)
    out_dtype = b.dtype
    with np.errstate(all="ignore"):
        nz64, b64 = np.asarray(nz, dtype=np.float64), np.asarray(b, dtype=np.float64)
        N = rl.N
        lu, u, bad = factor(sch, alpha, beta, nz64)
        flags = 2 if bad else 0
        r, rhat = b64.copy(), b64
        p, v, y = np.zeros(N), np.zeros(N), np.zeros(N)
        bn2 = M.dot_vec(b64, b64)
        one = np.float64(1.0)
        rho, rho_old, al, om = bn2, one, one, one
        tol2 = (np.float64(rtol) * np.float64(rtol)) * bn2
        rn2 = bn2
        done, iters = False, 0
        if bn2 == 0.0:
            done = True
        elif flags & 2:
            done = True
        elif M._bad(bn2):
            flags |= 2
            done = True
        enq = 0
        while not done and enq < max_iterations:
            enq += 1
            bk = (rho / rho_old) * (al / om)
            p = r + bk * (p - om * v)
            ph = apply(sch, lu, u, p)
            v = M.matvec(rl, alpha, beta, nz64, ph)
            rv = M.dot_rows(rhat, v)
            if M._bad(rv):
                flags |= 2
                break
            al = rho / rv
            s = r - al * v
            sn2 = M.dot_vec(s, s)
            if sn2 <= tol2:
                y = y + al * ph
                rn2 = sn2
                iters += 1
                done = True
                break
            sh = apply(sch, lu, u, s)
            t = M.matvec(rl, alpha, beta, nz64, sh)
            ts, tt = M.dot_rows(t, s), M.dot_rows(t, t)
            if M._bad(tt):
                flags |= 2
                break
            om = ts / tt
            y = (y + al * ph) + om * sh
            r = s - om * t
            rn2, rho_new = M.dot_vec(r, r), M.dot_vec(rhat, r)
            iters += 1
            if rn2 <= tol2:
                done = True
            else:
                rho_old, rho = rho, rho_new
                if M._bad(rho):
                    flags |= 2
                    break
        final = 2 if flags & 2 else (0 if done else 1)
        if final and not keep_unconverged:
            y = np.full(N, np.nan)
        return y.astype(out_dtype), {"flags": int(final), "iterations": int(iters), "resid": float(np.sqrt(rn2)), "bnorm": float(np.sqrt(bn2))}
