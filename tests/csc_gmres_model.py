"""numpy restatement of the restarted GMRES of the sparse consumer (csrc/fdjac_cscgmres.hip, fd_csc_solver_set_method): the cycle, the
CGS2 orthogonalisation with the order of every dot, the Givens step, the back substitution, the restart and every failure path --
operation for operation, so that the device's y, flags, iteration count, residual estimate, ||b|| and basis can be compared BIT FOR BIT.
The sums, the products and the three preconditioners are those of tests/csc_solve_model.py, csc_block_model.py and csc_ilu_model.py,
imported and unchanged.  Not a test file: tests/test_cscgmres_model_cpu.py and tests/test_gpu_cscgmres.py use it.

The algorithm (A = alpha I + beta J, right-preconditioned by M, y0 = 0, restart m):
  gamma = sqrt(dot_vec(r, r)) of r = b (first cycle) or r = b - A y (later cycles: gamma <= rtol ||b|| is converged, gamma^2 not finite a
  breakdown); v_0 = r / gamma; g = (gamma, 0, ...).
  Column j: z = M^-1 v_j; w = A z; h_i = dot_vec(w, v_i) for i = 0 .. j, all from the same w; w = ((w - h_0 v_0) - h_1 v_1) - ...; the
  same again for h'; H[i, j] = h_i + h'_i; H[j + 1, j] = sqrt(dot_vec(w, w)).  Any of them not finite: breakdown, the column does not
  count.  The stored rotations i = 0 .. j - 1 turn (a, b) = (col_i, col_i+1) into (c_i a + s_i b, c_i b - s_i a); then of
  (a, b) = (col_j, col_j+1): rho = sqrt(a a + b b); rho = 0: c = 1, s = 0; else c = a / rho, s = b / rho; rho, c or s not finite:
  breakdown.  R[j, j] = rho; g_j+1 = -s g_j; g_j = c g_j; the estimate is |g_j+1|; iterations + 1.  The cycle is over when the estimate
  <= rtol ||b|| (converged), H[j + 1, j] = 0, j + 1 = m, or the iterations have run out; otherwise v_j+1 = w / H[j + 1, j].
  The end of a cycle over K columns: t_i = (g_i - sum_{k > i} R[i, k] t_k) / R[i, i] for i = K - 1 .. 0, the sum from +0.0 with k
  ascending; a pivot that is zero or not finite: breakdown, nothing is added; else u = sum_i t_i v_i (i ascending from +0.0) and
  y = y + M^-1 u.
Final flags: 2 after a breakdown, else 1 when the iterations ran out, else 0.  After a failure y is NaN unless keep_unconverged."""
import numpy as np

import csc_solve_model as M
import csc_block_model as BM
import csc_ilu_model as IM

RESTART_MAX = 64
FAULTS = (None, "one_pass", "drop_last", "rotation_order")


def _finite(x):
    return bool(abs(x) < np.inf)


def preconditioner(rl, alpha, beta, nz64, precond):
    """-> (apply(x) -> M^-1 x, bad: a pivot of the set-up was zero or not finite).  precond: ("jacobi",), ("block", bs), ("ilu", bs)."""
    N = rl.N
    kind = precond[0]
    if kind == "jacobi":
        d = np.where(rl.diag >= 0, alpha + beta * nz64[np.maximum(rl.diag, 0)], np.float64(alpha)) if rl.nnz else np.full(N, np.float64(alpha))
        bad = not np.all((np.abs(d) > 0.0) & (np.abs(d) < np.inf))
        return (lambda x: x / d), bad
    if kind == "block":
        planes, bad = BM.block_inverses(rl.colptr, rl.rowval, N, alpha, beta, nz64, int(precond[1]))
        return (lambda x: BM.apply_planes(planes, x)), bad
    assert kind == "ilu"
    sch = IM.Schedule(rl, int(precond[1]))
    lu, u, bad = IM.factor(sch, alpha, beta, nz64)
    return (lambda x: IM.apply(sch, lu, u, x)), bad


def solve(rl, alpha, beta, nz, b, rtol=1e-10, max_iterations=500, keep_unconverged=False, restart=30, precond=("jacobi",), fault=None,
          trace=None):
    """(alpha I + beta J) y = b as fd_csc_solve_async computes it after fd_csc_solver_set_method(solver, FD_CSC_METHOD_GMRES, restart).
    Returns (y in b's dtype, {"flags", "iterations", "resid", "bnorm"}).  trace: a dict that receives "est" (per cycle the estimates,
    gamma first), "gammas" (every cycle's gamma), and the last cycle's "V" (the basis vectors formed, as rows), "H" (restart columns of
    restart + 1, as rows) and "len".  fault: one of FAULTS -- a deliberately wrong variant, for the tests of the tests."""
    assert 1 <= int(restart) <= RESTART_MAX and fault in FAULTS
    m = int(restart)
    out_dtype = b.dtype
    with np.errstate(all="ignore"):
        nz64, b64 = np.asarray(nz, dtype=np.float64), np.asarray(b, dtype=np.float64)
        alpha, beta = np.float64(alpha), np.float64(beta)
        N = rl.N
        apply, bad = preconditioner(rl, alpha, beta, nz64, precond)
        flags = 2 if bad else 0
        y = np.zeros(N)
        bn2 = M.dot_vec(b64, b64)
        gamma = np.sqrt(bn2)
        tol = np.float64(rtol) * gamma
        resid = gamma
        iters = 0
        done = ran_out = False
        if bn2 == 0.0 or flags & 2:
            done = True
        elif M._bad(bn2):
            flags |= 2
            done = True
        r = b64.copy()
        est_hist, gammas = [], []
        V = np.zeros((m + 1, N))
        H = np.zeros((m, m + 1))
        K = 0
        while not done:
            # ---- a cycle ----
            gammas.append(float(gamma))
            est_hist.append([float(gamma)])
            V[0] = r / gamma
            R = np.zeros((m, m + 1))
            c, s, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
            g[0] = gamma
            K = 0
            close = False
            for j in range(m):
                z = apply(V[j])
                w = M.matvec(rl, alpha, beta, nz64, z)
                hsum = np.zeros(j + 1)
                for _pass in range(1 if fault == "one_pass" else 2):
                    h = np.array([M.dot_vec(w, V[i]) for i in range(j + 1)])
                    for i in range(j + 1):
                        w = w - h[i] * V[i]
                    hsum = hsum + h if _pass else h
                hn = np.sqrt(M.dot_vec(w, w))
                col = np.zeros(m + 1)
                col[:j + 1] = hsum
                col[j + 1] = hn
                H[j] = col
                bad = not (_finite(hn) and np.all(np.abs(hsum) < np.inf))
                if not bad:
                    order = range(j - 1, -1, -1) if fault == "rotation_order" else range(j)
                    for i in order:
                        a_, b_ = col[i], col[i + 1]
                        col[i] = c[i] * a_ + s[i] * b_
                        col[i + 1] = c[i] * b_ - s[i] * a_
                    a_, b_ = col[j], col[j + 1]
                    rho = np.sqrt(a_ * a_ + b_ * b_)
                    cj, sj = (a_ / rho, b_ / rho) if rho != 0.0 else (np.float64(1.0), np.float64(0.0))
                    bad = not (_finite(rho) and _finite(cj) and _finite(sj))
                if bad:
                    flags |= 2
                    close = True
                    break
                col[j], col[j + 1] = rho, 0.0
                R[j] = col
                c[j], s[j] = cj, sj
                gj = g[j]
                g[j] = cj * gj
                g[j + 1] = -sj * gj
                est = abs(g[j + 1])
                resid = est
                est_hist[-1].append(float(est))
                K = j + 1
                iters += 1
                conv = bool(est <= tol)
                if not conv and iters >= max_iterations:
                    ran_out = True
                if conv or ran_out:
                    close = True
                if conv or hn == 0.0 or K == m or iters >= max_iterations:
                    break
                V[j + 1] = w / hn
            # ---- the end of the cycle ----
            t = np.zeros(m)
            bad = False
            for i in range(K - 1, -1, -1):
                acc = np.float64(0.0)
                for k in range(i + 1, K):
                    acc = acc + R[k, i] * t[k]
                piv = R[i, i]
                bad = bad or M._bad(piv)
                t[i] = (g[i] - acc) / piv
            if bad:
                flags |= 2
                close = True
            elif K > 0:
                u = np.zeros(N)
                for i in range(K - 1 if fault == "drop_last" else K):
                    u = u + t[i] * V[i]
                y = y + apply(u)
            if close:
                break
            r = b64 - M.matvec(rl, alpha, beta, nz64, y)
            g2 = M.dot_vec(r, r)
            gamma = np.sqrt(g2)
            resid = gamma
            if not _finite(g2):
                flags |= 2
                break
            if gamma <= tol:
                break
        if trace is not None:
            trace.update(est=est_hist, gammas=gammas, V=V.copy(), H=H.copy(), len=K)
        final = 2 if flags & 2 else (1 if ran_out else 0)
        if final and not keep_unconverged:
            y = np.full(N, np.nan)
        return y.astype(out_dtype), {"flags": int(final), "iterations": int(iters), "resid": float(resid), "bnorm": float(np.sqrt(bn2))}
