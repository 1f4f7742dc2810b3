"""numpy restatement of the WARM START of the sparse and the matrix-free consumer (fd_csc_solve_from_async, fd_jfnk_solve_from_async):
BiCGStab and restarted GMRES from an initial guess y0, operation for operation, so that the device's y, flags, iteration count,
resid and ||b|| can be compared BIT FOR BIT.  Not a test file: tests/test_warm_model_cpu.py and tests/test_gpu_warm_start.py use it.

THE RECURRENCES BELOW ARE CLOSE COPIES of csc_solve_model.solve (and its twins in csc_block_model / csc_ilu_model),
csc_gmres_model.solve and jfnk_model.gmres with the accumulator and the first residual changed.  The duplication is deliberate: the
existing model modules are yardsticks that the existing tests import and stay as they are; tests/test_warm_model_cpu.py pins every
recurrence here to them bit for bit (y0 = None and y0 = zeros).  Every primitive -- the row lists, the products, the sums, the three
preconditioners, the matrix-free operator, the lent factorisation -- is imported from those modules and not restated.

The start (both consumers, both methods; A = alpha I + beta J or the matrix-free operator):
  w = A y0        the sparse consumer: csc_solve_model.matvec on (double)y0, kept in Float64; the matrix-free one: one application of
                  jfnk_model.operator with z = y0 (the dot's order by jvp_enqueue's rule on x and the caller's y0)
  r0 = b - w      one subtraction per element; ||b||^2 and ||r0||^2 are csc_solve_model.dot_vec
  the stopping rule stays relative to b: tol^2 = rtol^2 ||b||^2 (GMRES inside a solve: rtol ||b||, as before)
  b = 0: y = 0, no iteration, whatever y0 holds.  A bad preconditioner pivot: breakdown.  ||b||^2 or ||r0||^2 not finite: breakdown
  (a NaN in y0 ends here); under the keep policy y is y0 then.  ||r0||^2 <= tol^2: y = y0 exactly, 0 iterations, resid = ||r0||.
  BiCGStab: r = rhat = r0, rho = ||r0||^2, p = v = 0, the accumulator starts at (double)y0.  GMRES: the first cycle opens on r0 with
  gamma = ||r0||, the accumulator at (double)y0; later restarts are unchanged.
Where the two consumers differ (the sparse start is ONE kernel, the matrix-free one checks first): the sparse consumer forms r0 whatever
the checks find, so its resid is ||r0|| after a bad pivot too (||b|| = 0 after b = 0); the matrix-free consumer applies nothing once
its opening kernel has ended the solve (b = 0, a bad pivot, ||b||^2 not finite) and reports ||b|| as the cold start does -- with a
preconditioner the host knows before it enqueues the product and does not count one; without one it is enqueued, counted and ignored.
FAULTS (deliberately wrong variants, for the tests of the tests): "tol_r0" (the tolerance relative to ||r0||), "forget_y0" (the result
lacks y0: the accumulator starts at 0), "rhat_b" (BiCGStab's shadow residual is b, not r0)."""
import numpy as np

import csc_gmres_model as G
import csc_solve_model as M
import jfnk_model as JM
import jfnk_pc_model as PM

FAULTS = (None, "tol_r0", "forget_y0", "rhat_b")


def _status(final, iters, resid, bn2):
    return {"flags": int(final), "iterations": int(iters), "resid": float(resid), "bnorm": float(np.sqrt(bn2))}


# ---- BiCGStab (csc_solve_model.solve with `apply` for the division, from y0) ----------------------------------------------------------
def bicgstab(rl, alpha, beta, nz, b, y0=None, rtol=1e-10, max_iterations=500, keep_unconverged=False, precond=("jacobi",), fault=None):
    assert fault in FAULTS
    out_dtype = b.dtype
    with np.errstate(all="ignore"):
        nz64, b64 = np.asarray(nz, dtype=np.float64), np.asarray(b, dtype=np.float64)
        alpha, beta = np.float64(alpha), np.float64(beta)
        N = rl.N
        apply, bad = G.preconditioner(rl, alpha, beta, nz64, precond)
        flags = 2 if bad else 0
        bn2 = M.dot_vec(b64, b64)
        if y0 is None:
            r, rhat, y, rn2 = b64.copy(), b64, np.zeros(N), bn2
        else:
            y064 = np.asarray(y0, dtype=np.float64)
            r = b64 - M.matvec(rl, alpha, beta, nz64, y064)
            rhat = b64 if fault == "rhat_b" else r.copy()
            y = np.zeros(N) if fault == "forget_y0" else y064.copy()
            rn2 = M.dot_vec(r, r)
            if bn2 == 0.0:
                rn2, y = bn2, np.zeros(N)
        p, v = np.zeros(N), np.zeros(N)
        one = np.float64(1.0)
        rho, rho_old, al, om = rn2, one, one, one
        tol2 = (np.float64(rtol) * np.float64(rtol)) * (rn2 if fault == "tol_r0" else bn2)
        done, iters = False, 0
        if bn2 == 0.0:
            done = True
        elif flags & 2:
            done = True
        elif not (G._finite(bn2) and G._finite(rn2)):
            flags |= 2
            done = True
        elif y0 is not None and rn2 <= (np.float64(rtol) * np.float64(rtol)) * bn2 and fault != "tol_r0":
            done = True
        enq = 0
        while not done and enq < max_iterations:
            enq += 1
            bk = (rho / rho_old) * (al / om)
            p = r + bk * (p - om * v)
            ph = apply(p)
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
            sh = apply(s)
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
        return y.astype(out_dtype), _status(final, iters, np.sqrt(rn2), bn2)


# ---- GMRES (jfnk_model.gmres, from y0) ------------------------------------------------------------------------------------------------
def gmres(product, apply, pre_bad, b, y0=None, rtol=1e-10, max_iterations=500, keep_unconverged=False, restart=30, checks_first=False,
          fault=None, trace=None):
    """product(v, kind, j) -> A v: kind "start" (w = A y0), "step" (column j's product), "resid" (the explicit residual's);
    apply(x) -> M^-1 x.  checks_first: the matrix-free consumer's order (nothing is applied once the opening checks have ended the
    solve); otherwise the sparse consumer's (the start forms r0 whatever the checks find)."""
    assert 1 <= int(restart) <= G.RESTART_MAX and fault in FAULTS
    m = int(restart)
    with np.errstate(all="ignore"):
        b64 = np.asarray(b, dtype=np.float64)
        N = b64.size
        flags = 2 if pre_bad else 0
        y = np.zeros(N)
        bn2 = M.dot_vec(b64, b64)
        done = ran_out = False
        if bn2 == 0.0 or flags & 2:
            done = True
        elif M._bad(bn2):
            flags |= 2
            done = True
        r, g2 = b64.copy(), bn2
        if y0 is not None:
            y064 = np.asarray(y0, dtype=np.float64)
            if not (checks_first and done):
                r = b64 - product(y064, "start", 0)
                g2 = M.dot_vec(r, r)
            if not done or ((flags & 2) and bn2 != 0.0):      # (the iterate under the keep policy: y0, but 0 after b = 0)
                y = np.zeros(N) if fault == "forget_y0" else y064.copy()
            if bn2 == 0.0:
                g2 = bn2
            if not done:
                if not G._finite(g2):
                    flags |= 2
                    done = True
                elif g2 <= (np.float64(rtol) * np.float64(rtol)) * bn2 and fault != "tol_r0":
                    done = True
        gamma = np.sqrt(g2)
        tol = np.float64(rtol) * (gamma if fault == "tol_r0" else np.sqrt(bn2))
        resid = gamma
        iters = 0
        est_hist, gammas = [], []
        V = np.zeros((m + 1, N))
        H = np.zeros((m, m + 1))
        K = 0
        while not done:
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
                w = product(z, "step", j)
                hsum = np.zeros(j + 1)
                for _pass in range(2):
                    h = np.array([M.dot_vec(w, V[i]) for i in range(j + 1)])
                    for i in range(j + 1):
                        w = w - h[i] * V[i]
                    hsum = hsum + h if _pass else h
                hn = np.sqrt(M.dot_vec(w, w))
                col = np.zeros(m + 1)
                col[:j + 1] = hsum
                col[j + 1] = hn
                H[j] = col
                bad = not (G._finite(hn) and np.all(np.abs(hsum) < np.inf))
                if not bad:
                    for i in range(j):
                        a_, b_ = col[i], col[i + 1]
                        col[i] = c[i] * a_ + s[i] * b_
                        col[i + 1] = c[i] * b_ - s[i] * a_
                    a_, b_ = col[j], col[j + 1]
                    rho = np.sqrt(a_ * a_ + b_ * b_)
                    cj, sj = (a_ / rho, b_ / rho) if rho != 0.0 else (np.float64(1.0), np.float64(0.0))
                    bad = not (G._finite(rho) and G._finite(cj) and G._finite(sj))
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
                for i in range(K):
                    u = u + t[i] * V[i]
                y = y + apply(u)
            if close:
                break
            r = b64 - product(y, "resid", 0)
            g2 = M.dot_vec(r, r)
            gamma = np.sqrt(g2)
            resid = gamma
            if not G._finite(g2):
                flags |= 2
                break
            if gamma <= tol:
                break
        if trace is not None:
            trace.update(est=est_hist, gammas=gammas, V=V.copy(), H=H.copy(), len=K)
        final = 2 if flags & 2 else (1 if ran_out else 0)
        if final and not keep_unconverged:
            y = np.full(N, np.nan)
        return y, _status(final, iters, resid, bn2)


# ---- the sparse consumer --------------------------------------------------------------------------------------------------------------
def csc_solve(rl, alpha, beta, nz, b, y0=None, method="bicgstab", precond=("jacobi",), restart=30, rtol=1e-10, max_iterations=500,
              keep_unconverged=False, fault=None):
    """(alpha I + beta J) y = b as fd_csc_solve_from_async computes it from y0 (None: the cold start).  precond: ("jacobi",),
    ("block", bs), ("ilu", bs).  Returns (y in b's dtype, {"flags", "iterations", "resid", "bnorm"})."""
    if method == "bicgstab":
        return bicgstab(rl, alpha, beta, nz, b, y0, rtol, max_iterations, keep_unconverged, precond, fault)
    assert method == "gmres"
    with np.errstate(all="ignore"):
        nz64 = np.asarray(nz, dtype=np.float64)
        alpha, beta = np.float64(alpha), np.float64(beta)
        apply, bad = G.preconditioner(rl, alpha, beta, nz64, precond)
        y, st = gmres(lambda v, kind, j: M.matvec(rl, alpha, beta, nz64, v), apply, bad, b, y0, rtol, max_iterations, keep_unconverged, restart,
                      False, None if fault == "rhat_b" else fault)
        return y.astype(b.dtype), st


# ---- the matrix-free consumer ---------------------------------------------------------------------------------------------------------
def jfnk_solve(f, x, b, alpha, beta, y0=None, fdtype="forward", d=None, lent=None, rtol=1e-10, max_iterations=500, keep_unconverged=False,
               restart=30, num_cus=256, relstep=None, absstep=None, dir=1.0, f_in=None, x_aligned=True, y0_aligned=True, small_off=False,
               fault=None, trace=None):
    """(alpha I + beta J(x)) y = b as fd_jfnk_solve_from_async computes it from y0.  d: the diagonal, or lent = (rl, (alpha0, beta0, nz0),
    precond): a lent factorisation (jfnk_pc_model.factorisation), or neither.  trace also receives "applications" and
    "base_evaluations" as fd_jfnk_solver_counts counts them for this solve."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    napp = [0]
    own_z = d is not None or lent is not None          # z of a step is the solver's own vector (always on a pair)

    def product(v, kind, j):
        napp[0] += 1
        z_al = y0_aligned if kind == "start" else (True if (kind == "resid" or own_z) else (j * N) % 2 == 0)
        return JM.operator(f, x, v, alpha, beta, fdtype, JM.dot_order(N, x_aligned, z_al, small_off), num_cus, relstep, absstep, dir, f_in)

    if lent is not None:
        rl, (a0, b0, nz0), precond = lent
        apply, pre_bad = PM.factorisation(rl, a0, b0, nz0, precond)
    elif d is not None:
        d64 = np.asarray(d, dtype=np.float64)
        with np.errstate(all="ignore"):
            pre_bad = not np.all((np.abs(d64) > 0.0) & (np.abs(d64) < np.inf))
        apply = lambda v: v / d64          # noqa: E731
    else:
        apply, pre_bad = (lambda v: v), False
    y, st = gmres(product, apply, pre_bad, b, y0, rtol, max_iterations, keep_unconverged, restart, True, None if fault == "rhat_b" else fault, trace)
    with np.errstate(all="ignore"):
        b64 = np.asarray(b, dtype=np.float64)
        bn2 = M.dot_vec(b64, b64)
        ended = bool(bn2 == 0.0 or pre_bad or M._bad(bn2))          # the opening kernel has ended the solve
    base = 1 if (fdtype == "forward" and f_in is None) else 0
    if y0 is not None and ended:
        if own_z:
            base = 0          # the host has read the verdict: nothing of the operator is enqueued
        else:
            napp[0] += 1      # enqueued behind the opening kernel, and ignored
    if trace is not None:
        trace["applications"] = napp[0]
        trace["base_evaluations"] = base
    return y, st
