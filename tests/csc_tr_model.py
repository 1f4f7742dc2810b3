"""numpy restatement of the trust-region consumer (csrc/fdjac_csctr.hip): the row lists (csc_solve_model.RowLists), the product
(H + lambda I) v with its summation orders (long rows by the fixed tree), the order of every dot, the whole Steihaug-Toint recurrence with
its exits and failure handling, and the status -- operation for operation, so that the device's results can be compared BIT FOR BIT.
No FMA anywhere.  Not a test file: tests/test_csctr_model_cpu.py, tests/test_gpu_csctr.py and tests/csctr_switch_child.py use it."""
import numpy as np

from csc_solve_model import LONG, RowLists, block_sum, dot_rows, dot_vec, random_band_pattern, strided_sum

NORM_IDENTITY, NORM_DIAG = 0, 1
EXIT_INTERIOR, EXIT_BOUNDARY, EXIT_NEGATIVE, EXIT_UNBOUNDED = 0, 1, 2, 3


# ---- symmetric patterns with values (0-based colptr / rowval, int64) ------------------------------------------------------------------
def _offdiag(N, half, per_col, seed, long=None):
    """The strictly upper pairs (lo < hi) of the pattern of A + A^T for A = random_band_pattern(N, half, per_col, seed), with values
    0.5 u, u uniform in [-1, 1]; the rows named in `long` ({row: length}, the diagonal counted) are padded to that length with random
    partners whose values are u / length (so a padded row's absolute sum grows by at most 1)."""
    colptr, rowval, _ = random_band_pattern(N, half, per_col, seed)
    cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
    off = rowval != cols
    key = np.unique(np.minimum(rowval[off], cols[off]) * N + np.maximum(rowval[off], cols[off]))
    rng = np.random.default_rng(seed + 1000)
    vals = 0.5 * rng.uniform(-1.0, 1.0, key.size)
    keys, extra_vals = set(key.tolist()), {}
    for i, length in sorted((long or {}).items()):
        have = 1 + sum(1 for k in keys if k // N == i or k % N == i) + sum(1 for k in extra_vals if k // N == i or k % N == i)
        for j in rng.permutation(N):
            if have >= length:
                break
            k = int(min(i, j) * N + max(i, j))
            if j == i or j in long or k in keys or k in extra_vals:      # (no partner among the padded rows: their lengths stay exact)
                continue
            extra_vals[k] = rng.uniform(-1.0, 1.0) / length
            have += 1
    if extra_vals:
        key = np.concatenate([key, np.fromiter(extra_vals.keys(), dtype=np.int64)])
        vals = np.concatenate([vals, np.fromiter(extra_vals.values(), dtype=np.float64)])
    return key // N, key % N, vals


def abs_row_sums(N, half, per_col, seed, long=None):
    """sum_{j != i} |H_ij| of sym_band's matrix: what a caller needs to choose a dominant diagonal."""
    lo, hi, vals = _offdiag(N, half, per_col, seed, long)
    s = np.zeros(N)
    np.add.at(s, lo, np.abs(vals))
    np.add.at(s, hi, np.abs(vals))
    return s


def sym_band(N, half, per_col, seed, diag, long=None):
    """The pattern of A + A^T for a random_band_pattern, every diagonal entry stored, symmetric values (H_ij = H_ji bit for bit), the
    diagonal `diag` (a vector of N), optionally rows-and-columns padded to a chosen length (`long`: {row: length}).
    Returns (colptr, rowval, nzval, N)."""
    lo, hi, vals = _offdiag(N, half, per_col, seed, long)
    d = np.arange(N, dtype=np.int64)
    r = np.concatenate([lo, hi, d])
    c = np.concatenate([hi, lo, d])
    v = np.concatenate([vals, vals, np.asarray(diag, dtype=np.float64)])
    order = np.lexsort((r, c))                            # by column, rows ascending within a column
    colptr = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=N))]).astype(np.int64)
    return colptr, r[order].astype(np.int64), v[order], N


BAND = dict(N=3000, half=40, per_col=4, seed=11)
LONG_ROWS = {100: 33, 1500: 300, 2999: 2500}


def _dominant_diagonal(long):
    """|H_ii| = sum_{j != i} |H_ij| + 1 + u, u uniform in [0, 1): strictly dominant, Gershgorin's discs stay right of 1."""
    return abs_row_sums(long=long, **BAND) + 1.0 + np.random.default_rng(5).uniform(0.0, 1.0, BAND["N"])


def named_case(name):
    """(colptr, rowval, nzval, N) of `spd`, `spd_long` (rows of 33, 300 and 2500 entries) and `indef` (`spd` with every tenth diagonal
    entry's sign flipped: H_jj <= -1 there, so lambda_min <= H_jj < 0)."""
    if name == "spd":
        return sym_band(diag=_dominant_diagonal(None), **BAND)
    if name == "spd_long":
        return sym_band(diag=_dominant_diagonal(LONG_ROWS), long=LONG_ROWS, **BAND)
    if name == "indef":
        diag = _dominant_diagonal(None)
        diag[3::10] = -diag[3::10]
        return sym_band(diag=diag, **BAND)
    raise KeyError(name)


def tiny_case(N):
    """N = 1, 2, 3: the full N x N pattern, symmetric positive definite values."""
    A = {1: [[2.0]], 2: [[2.0, -0.5], [-0.5, 1.5]], 3: [[2.0, -0.5, 0.25], [-0.5, 1.5, 0.75], [0.25, 0.75, 3.0]]}[N]
    A = np.array(A)
    colptr = (np.arange(N + 1) * N).astype(np.int64)
    return colptr, np.tile(np.arange(N, dtype=np.int64), N), A.T.reshape(-1).copy(), N


# ---- the product ----------------------------------------------------------------------------------------------------------------------
def row_sums(rl, nz, v):
    """H v: rows of at most LONG entries left to right in ascending column from +0.0; longer ones: thread t adds entries t, t + 256,
    ..., then block_sum."""
    prods = nz[rl.row_slot] * v[rl.row_col]
    acc = np.zeros(rl.N)
    short = rl.lens <= LONG
    maxlen = int(rl.lens[short].max()) if short.any() else 0
    for k in range(maxlen):
        rows = np.nonzero(short & (rl.lens > k))[0]
        acc[rows] = acc[rows] + prods[rl.row_ptr[rows] + k]
    for r in np.nonzero(~short)[0]:
        acc[r] = block_sum(strided_sum(prods[rl.row_ptr[r]:rl.row_ptr[r + 1]]))
    return acc


def matvec(rl, lam, nz, v):
    """fd_csc_tr_matvec_async: y_r = (row sum) + lambda * v_r."""
    with np.errstate(all="ignore"):
        nz, v = np.asarray(nz, dtype=np.float64), np.asarray(v, dtype=np.float64)
        return row_sums(rl, nz, v) + np.float64(lam) * v


# ---- Steihaug-Toint -------------------------------------------------------------------------------------------------------------------
def _not_finite(x):
    return not (abs(x) < np.inf)


def precond(rl, lam, kind, nz):
    """m: ones (kind 0) or |H_jj| + lambda with a diagonal that is not stored counted as 0 (kind 1)."""
    if kind == NORM_IDENTITY:
        return np.ones(rl.N)
    hjj = np.where(rl.diag >= 0, nz[np.maximum(rl.diag, 0)], 0.0) if rl.nnz else np.zeros(rl.N)
    return np.abs(hjj) + np.float64(lam)


def step(rl, lam, radius, kind, nz, g, rtol=1e-10, max_iterations=500, keep_unconverged=False, trace=None):
    """min g.y + 1/2 y.(H + lam I) y, ||y||_W <= radius, as fd_csc_tr_step_async computes it.  Returns (y, r_out, status),
    status = {"flags", "exit", "iterations", "resid", "g_norm", "step_norm", "pred"}.  `trace`: a list that receives every iterate y_k."""
    with np.errstate(all="ignore"):
        nz, g = np.asarray(nz, dtype=np.float64), np.asarray(g, dtype=np.float64)
        lam = np.float64(lam)
        delta2 = np.float64(radius) * np.float64(radius)
        N = rl.N
        m = precond(rl, lam, kind, nz)
        flags, exit_kind = 0, 0
        if kind == NORM_DIAG and not np.all((np.abs(m) > 0.0) & (np.abs(m) < np.inf)):
            flags |= 2
        r = g.copy()
        y = np.zeros(N)
        z = r / m
        p = -z
        gamma, rho0, ppp = dot_vec(r, z), dot_vec(r, r), dot_vec(m * p, p)
        pyp = pyy = np.float64(0.0)
        rho = rho0
        tol2 = (np.float64(rtol) * np.float64(rtol)) * rho0
        done, iters = False, 0
        if rho0 == 0.0:
            done = True
        elif flags & 2:
            done = True
        elif _not_finite(gamma):
            flags |= 2
            done = True
        enq = 0
        while not done and enq < max_iterations:
            enq += 1
            q = row_sums(rl, nz, p) + lam * p
            kappa = dot_rows(p, q)
            d = delta2 - pyy
            tau = d / (pyp + np.sqrt(pyp * pyp + ppp * d))
            if _not_finite(kappa):
                flags |= 2
                break
            if kappa <= 0.0:
                if _not_finite(delta2):
                    exit_kind = EXIT_UNBOUNDED
                    flags |= 2
                    break
                exit_kind, alpha = EXIT_NEGATIVE, tau
            else:
                alpha = gamma / kappa
                if pyy + 2.0 * alpha * pyp + alpha * alpha * ppp >= delta2:
                    exit_kind, alpha = EXIT_BOUNDARY, tau
            y = y + alpha * p
            r = r + alpha * q
            z = r / m
            gamma_new, rho = dot_vec(r, z), dot_vec(r, r)
            iters += 1
            if trace is not None:
                trace.append(y.copy())
            if exit_kind != 0 or rho <= tol2:
                done = True
                break
            if _not_finite(gamma_new):
                flags |= 2
                break
            beta = gamma_new / gamma
            gamma = gamma_new
            p = -z + beta * p
            ppp, pyp, pyy = dot_vec(m * p, p), dot_vec(m * y, p), dot_vec(m * y, y)
        final = 2 if flags & 2 else (0 if done else 1)      # bit 1: breakdown; bit 0: the iterations ran out
        yw2 = dot_vec(m * y, y)
        pred = np.float64(-0.5) * dot_vec(y, g + r)
        if final and not keep_unconverged:
            y, r = np.full(N, np.nan), np.full(N, np.nan)
        return y, r, {"flags": int(final), "exit": int(exit_kind), "iterations": int(iters), "resid": float(np.sqrt(rho)),
                      "g_norm": float(np.sqrt(rho0)), "step_norm": float(np.sqrt(yw2)), "pred": float(pred)}


def same_status(a, b):
    """Equality of two status records with the four scalars compared BIT FOR BIT (NaN equals NaN of the same bits' class)."""
    if set(a) != set(b):
        return False
    for k in a:
        if isinstance(a[k], float) or isinstance(b[k], float):
            x, y = np.float64(a[k]), np.float64(b[k])
            if not (x.view(np.uint64) == y.view(np.uint64) or (np.isnan(x) and np.isnan(y))):
                return False
        elif a[k] != b[k]:
            return False
    return True
