"""numpy restatement of the block-Jacobi preconditioner of the sparse consumer (csrc/fdjac_cscsolve.hip: k_cs_binv, k_cs_bapply and the
PC = 1 instances of the vector kernels): the gather of the diagonal blocks, their inversion and the apply, operation for operation, and
the BiCGStab recurrence around them with the dots and products of tests/csc_solve_model.py -- so that the device's inverses, y,
iteration count, residual norm and flags can be compared BIT FOR BIT.  Not a test file: tests/test_cscblock_model_cpu.py and
tests/test_gpu_cscblock.py use it.

Blocks: the uniform ranges [k bs, min((k + 1) bs, N)).  B_k = alpha I + beta J[rows of k, columns of k] from the stored entries: a
stored diagonal is alpha + beta * nzval, any other stored entry beta * nzval (no addition), an entry that is not stored 0, a diagonal
that is not stored alpha.

Inversion of a block of n rows: Gauss-Jordan on [B | I] with partial pivoting.  Step j = 0 .. n - 1:
  best = j; for i = j + 1 .. n - 1: if |a[i, j]| > |a[best, j]|: best = i     (strictly greater: the lowest row wins a tie; a NaN
         never replaces, and a NaN a[j, j] is never replaced);
  piv = a[best, j]; zero or not finite: breakdown (the solve ends with flags 2 and no iteration), the arithmetic goes on regardless;
  rows j and best are swapped; every row i != j: f_i = a[i, j] / piv, a[i, l] = a[i, l] - f_i * a[j, l]; then row j:
  a[j, l] = a[j, l] / piv.  Two rows that are equal bit for bit leave an exact zero row behind (f = 1), hence a zero pivot.
The inverse is the right half.  (The device leaves the columns l <= j of the left half alone from step j on: they are not read again.)

Apply: out[i] = sum_c Minv[i - b0, c] * x[b0 + c], c = 0 .. n - 1 ascending from +0.0, one multiply and one add per term."""
import numpy as np

import csc_solve_model as M


# ---- the family of the tests: a grid of cells with m strongly coupled unknowns per cell ------------------------------------------------
def reaction_diffusion(nx, ny, m, k, cond, skew, seed):
    """J = D + R on nx x ny cells with m species per cell, the species the fastest index.  D: the 5-point Laplacian per species
    (-4 c_s on the diagonal, c_s towards every neighbouring cell that exists), c = linspace(0.5, 1.5, m).  R: block-diagonal, per cell
    -k (Q diag(lam) Q^T + skew K), Q a random orthogonal matrix, lam log-spaced in [1 / cond, 1], K = (G - G^T) / 2 of a standard normal
    G.  Returns 0-based (colptr, rowval, nzval, N), rows ascending within a column, the cell's block stored densely."""
    rng = np.random.default_rng(seed)
    ncell, N = nx * ny, nx * ny * m
    c = np.linspace(0.5, 1.5, m)
    lam = np.logspace(-np.log10(cond), 0.0, m)
    G = rng.standard_normal((ncell, m, m))
    Q = np.empty_like(G)
    for i in range(ncell):
        Q[i] = np.linalg.qr(G[i])[0]
    H = rng.standard_normal((ncell, m, m))
    K = 0.5 * (H - np.swapaxes(H, 1, 2))
    R = -k * (np.einsum("cik,k,cjk->cij", Q, lam, Q) + skew * K)
    R[:, np.arange(m), np.arange(m)] += -4.0 * c                    # the Laplacian's diagonal
    cell = np.arange(ncell)
    ci, cj = cell % nx, cell // nx
    # per column (cell, s): [cell - nx, cell - 1, the m rows of the cell, cell + 1, cell + nx] -- ascending rows
    rows = np.full((ncell, m, m + 4), -1, dtype=np.int64)
    vals = np.zeros((ncell, m, m + 4))
    s = np.arange(m)
    for slot, (nb, ok) in ((0, (cell - nx, cj > 0)), (1, (cell - 1, ci > 0)), (m + 2, (cell + 1, ci < nx - 1)), (m + 3, (cell + nx, cj < ny - 1))):
        rows[:, :, slot] = np.where(ok[:, None], nb[:, None] * m + s[None, :], -1)
        vals[:, :, slot] = c[None, :]
    rows[:, :, 2:m + 2] = (cell[:, None] * m + s[None, :])[:, None, :]          # row (cell, t) for every column s
    vals[:, :, 2:m + 2] = np.swapaxes(R, 1, 2)                                    # column s, row t: R[t, s]
    keep = rows >= 0
    colptr = np.concatenate([[0], np.cumsum(keep.reshape(N, -1).sum(axis=1))]).astype(np.int64)
    return colptr, rows[keep].astype(np.int64), vals[keep], N


def block_tridiag_pattern(nblk, bs):
    """Block-tridiagonal with dense bs x bs blocks (the block-coupled configuration's shape): interior rows hold 3 bs entries."""
    N = nblk * bs
    j = np.arange(N)
    lo = np.maximum(j // bs - 1, 0) * bs
    hi = np.minimum(j // bs + 2, nblk) * bs
    colptr = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64)
    rowval = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]).astype(np.int64)
    return colptr, rowval, N


# ---- gather ---------------------------------------------------------------------------------------------------------------------------
def gather_blocks(colptr, rowval, N, alpha, beta, nz, bs, idx_base=0):
    """-> (nblk, bs, bs) Float64; the last block's rows and columns beyond its length are zero (and not part of it).  colptr / rowval
    of any integer type, as fd_csc_solver_create takes them: idx_base = 1 for one-based offsets and rows."""
    assert idx_base in (0, 1)
    colptr, rowval = np.asarray(colptr).astype(np.int64) - idx_base, np.asarray(rowval).astype(np.int64) - idx_base
    assert colptr.size == N + 1 and colptr[0] == 0 and colptr[-1] == rowval.size and (rowval.size == 0 or (rowval.min() >= 0 and rowval.max() < N))
    nz64 = np.asarray(nz, dtype=np.float64)
    alpha, beta = np.float64(alpha), np.float64(beta)
    nblk = (N + bs - 1) // bs
    B = np.zeros((nblk, bs, bs))
    i = np.arange(N)
    B[i // bs, i % bs, i % bs] = alpha
    cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
    inb = (rowval // bs) == (cols // bs)
    r, c, v = rowval[inb], cols[inb], nz64[inb]
    with np.errstate(all="ignore"):
        B[c // bs, r % bs, c % bs] = np.where(r == c, alpha + beta * v, beta * v)
    return B


# ---- inversion ------------------------------------------------------------------------------------------------------------------------
def invert_blocks(B):
    """(nb, n, n) -> (the inverses (nb, n, n), bad (nb,): a pivot of that block was zero or not finite)."""
    nb, n = B.shape[0], B.shape[1]
    A = np.concatenate([np.array(B, dtype=np.float64), np.broadcast_to(np.eye(n), (nb, n, n))], axis=2)
    bad = np.zeros(nb, dtype=bool)
    ar = np.arange(nb)
    with np.errstate(all="ignore"):
        for j in range(n):
            mag = np.abs(A[:, j:, j])
            cand = np.where(np.isnan(mag), -1.0, mag)
            best = np.where(np.isnan(mag[:, 0]), 0, np.argmax(cand, axis=1)) + j      # the first of the largest; a NaN head stays
            piv = A[ar, best, j]
            bad |= ~((np.abs(piv) > 0.0) & (np.abs(piv) < np.inf))
            rj, rb = A[ar, j, :].copy(), A[ar, best, :].copy()
            A[ar, best, :] = rj
            A[ar, j, :] = rb
            f = A[:, :, j] / piv[:, None]
            new = A - f[:, :, None] * rb[:, None, :]
            new[:, j, :] = rb / piv[:, None]
            A = new
    return A[:, :, n:], bad


def block_inverses(colptr, rowval, N, alpha, beta, nz, bs, idx_base=0):
    """The planes the device keeps: (bs, N), [c, i] = Minv[i - b0, c]; and whether any pivot was bad."""
    B = gather_blocks(colptr, rowval, N, alpha, beta, nz, bs, idx_base)
    nfull, tail = N // bs, N % bs
    planes = np.zeros((bs, N))
    bad = False
    if nfull:
        inv, b = invert_blocks(B[:nfull])
        planes[:, :nfull * bs] = inv.transpose(2, 0, 1).reshape(bs, nfull * bs)
        bad = bool(b.any())
    if tail:
        inv, b = invert_blocks(B[nfull:, :tail, :tail])
        planes[:tail, nfull * bs:] = inv[0].T
        bad = bad or bool(b.any())
    return planes, bad


# ---- apply ----------------------------------------------------------------------------------------------------------------------------
def apply_planes(planes, x):
    bs, N = planes.shape
    i = np.arange(N)
    b0 = i // bs * bs
    n = np.minimum(bs, N - b0)
    acc = np.zeros(N)
    with np.errstate(all="ignore"):
        for c in range(bs):
            on = n > c
            acc[on] = acc[on] + planes[c, on] * x[b0[on] + c]
    return acc


# ---- BiCGStab -------------------------------------------------------------------------------------------------------------------------
def solve(rl, alpha, beta, nz, b, rtol=1e-10, max_iterations=500, keep_unconverged=False, precond=("block", 8)):
    """(alpha I + beta J) y = b as fd_csc_solve_async computes it after fd_csc_solver_set_preconditioner(solver, 1, bs); with
    precond = ("jacobi",) it is csc_solve_model.solve.  Returns (y in b's dtype, {"flags", "iterations", "resid", "bnorm"})."""
    if precond[0] == "jacobi":
        return M.solve(rl, alpha, beta, nz, b, rtol, max_iterations, keep_unconverged)
    assert precond[0] == "block" and 2 <= int(precond[1]) <= 32
    bs = int(precond[1])
    out_dtype = b.dtype
    with np.errstate(all="ignore"):
        nz64, b64 = np.asarray(nz, dtype=np.float64), np.asarray(b, dtype=np.float64)
        N = rl.N
        planes, bad = block_inverses(rl.colptr, rl.rowval, N, alpha, beta, nz64, bs)
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
            ph = apply_planes(planes, p)
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
            sh = apply_planes(planes, s)
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
