"""numpy restatement of the matrix-free consumer (csrc/fdjac_jfnk.hip, fd_jfnk_*): restarted GMRES on the finite-difference JVP,
operation for operation, so that the device's y, flags, iteration count, estimate, ||b|| and last basis can be compared BIT FOR BIT.
Not a test file: tests/test_jfnk_model_cpu.py and tests/test_gpu_jfnk.py use it.

  the cycle     gmres() below: the algorithm at the head of tests/csc_gmres_model.py word for word, with the operator and the
                preconditioner as callables (with csc_solve_model.matvec and the Jacobi diagonal plugged in it IS csc_gmres_model.solve,
                bit for bit: tests/test_jfnk_model_cpu.py).  The GMRES sums are csc_solve_model.dot_vec.
  the operator  A(x) z = alpha z + beta q,  q = jvp_model.jvp at eps = jvp_model.epsilon(jvp_model.dot(x, z, order)); w_e = alpha z_e +
                beta q_e, two multiplications and one addition.  f is a restatement from exact_model.py (jvp_cases.inputs hands it out).
  order         of dot(x, z), the only thing the JVP's routes differ in, by jvp_enqueue's own rule on the two operands (dot_order below):
                "small" up to kSmallN; above it "paired" when x and z both start on a pair, else "scalar".  With a diagonal z is the
                solver's own vector (always aligned; where v_j and d sit changes loads, not sums); without one z IS v_j = V + j N, so for
                an odd N the order alternates with j.  The explicit residual's product reads y (the solver's own).  apply(): x and the
                caller's z.  So q is always what fd_jvp_async returns for (x, z).
  the CU count  the large orders run on balanced_grid(ceil(N / 256), 8 num_cus) workgroups: a parameter, as in jvp_model.
FAULTS: csc_gmres_model's deliberately wrong variants and "close_order", which multiplies by beta before it divides by eps."""
import numpy as np

import csc_gmres_model as G
import csc_solve_model as M
import jvp_model as J

FAULTS = G.FAULTS + ("close_order",)
RESTART_MAX = G.RESTART_MAX


def dot_order(N, x_aligned, z_aligned=True, small_off=False):
    if N <= J.SMALL_N and not small_off:
        return "small"
    return "paired" if (x_aligned and z_aligned) else "scalar"


def operator(f, x, z, alpha, beta, fdtype, order, num_cus=256, relstep=None, absstep=None, dir=1.0, f_in=None, fault=None):
    """w = alpha z + beta q as fd_jfnk_apply_async computes it; order: the summation order of dot(x, z)."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = J.dot(x, z, order, num_cus)
        eps = J.epsilon(t, fdtype, relstep, absstep, dir)
        alpha, beta = np.float64(alpha), np.float64(beta)
        if fault == "close_order":
            e = np.float64(eps)
            ev = e * z
            if fdtype == "forward":
                base = f(x) if f_in is None else np.asarray(f_in, dtype=np.float64)
                return alpha * z + (beta * (f(x + ev) - base)) / e
            return alpha * z + (beta * (f(x + ev) - f(x - ev))) / (np.float64(2) * e)
        q = J.jvp(f, x, z, eps, fdtype, f_in)
        return alpha * z + beta * q


def gmres(product, apply, pre_bad, b, rtol=1e-10, max_iterations=500, keep_unconverged=False, restart=30, fault=None, trace=None):
    """The cycle of csc_gmres_model.solve with product(v, kind, j) -> A v (kind "step": column j's product of z = M^-1 v_j; "resid": the
    explicit residual's) and apply(x) -> M^-1 x; pre_bad: the preconditioner's set-up found a bad pivot.  Returns (y, status)."""
    assert 1 <= int(restart) <= RESTART_MAX and fault in FAULTS
    m = int(restart)
    with np.errstate(all="ignore"):
        b64 = np.asarray(b, dtype=np.float64)
        N = b64.size
        flags = 2 if pre_bad else 0
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
                bad = not (G._finite(hn) and np.all(np.abs(hsum) < np.inf))
                if not bad:
                    order = range(j - 1, -1, -1) if fault == "rotation_order" else range(j)
                    for i in order:
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
                for i in range(K - 1 if fault == "drop_last" else K):
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
        return y, {"flags": int(final), "iterations": int(iters), "resid": float(resid), "bnorm": float(np.sqrt(bn2))}


def solve(f, x, b, alpha, beta, fdtype="forward", d=None, rtol=1e-10, max_iterations=500, keep_unconverged=False, restart=30, num_cus=256,
          relstep=None, absstep=None, dir=1.0, f_in=None, x_aligned=True, small_off=False, fault=None, trace=None):
    """(alpha I + beta J(x)) y = b as fd_jfnk_solve_async computes it.  d: the diagonal of the right preconditioner or None; x_aligned:
    whether the device array starts on a pair (16 bytes); small_off: FDJAC_SMALL=0.  trace also receives "applications"."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    napp = [0]
    op_fault = fault if fault == "close_order" else None

    def product(v, kind, j):
        napp[0] += 1
        # z of a step: the solver's own vector behind a diagonal, v_j = V + j N in place without one; the residual reads the solver's y
        z_al = True if (kind == "resid" or d is not None) else (j * N) % 2 == 0
        order = dot_order(N, x_aligned, z_al, small_off)
        return operator(f, x, v, alpha, beta, fdtype, order, num_cus, relstep, absstep, dir, f_in, op_fault)

    if d is None:
        apply, pre_bad = (lambda v: v), False
    else:
        d64 = np.asarray(d, dtype=np.float64)
        with np.errstate(all="ignore"):
            pre_bad = not np.all((np.abs(d64) > 0.0) & (np.abs(d64) < np.inf))
        apply = lambda v: v / d64          # noqa: E731
    y, st = gmres(product, apply, pre_bad, b, rtol, max_iterations, keep_unconverged, restart, fault if fault != "close_order" else None, trace)
    if trace is not None:
        trace["applications"] = napp[0]
    return y, st


# ---- the analytic Jacobians of the built-in square families (the accuracy check's J_exact) ------------------------------------------
def jacobian_dense(family, prm, x):
    """d f / d x of tests/exact_model.py's tridiag / tridiag_nl / lap5 / lap5_nl at x, dense Float64."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    Jm = np.zeros((N, N))
    idx = np.arange(N)
    if family.startswith("tridiag"):
        Jm[idx, idx] = -2.0
        Jm[idx[1:], idx[:-1]] = 1.0
        Jm[idx[:-1], idx[1:]] = 1.0
        if family.endswith("_nl"):                       # + x_i^2 x_{i+1}
            xp = np.concatenate([x[1:], [0.0]])
            Jm[idx, idx] += 2.0 * x * xp
            Jm[idx[:-1], idx[1:]] += x[:-1] ** 2
        return Jm
    nx, ny = prm
    assert family.startswith("lap5") and nx * ny == N
    Jm[idx, idx] = -4.0
    for k in range(N):
        j, i = divmod(k, nx)
        if i > 0:
            Jm[k, k - 1] = 1.0
        if i + 1 < nx:
            Jm[k, k + 1] = 1.0
        if j > 0:
            Jm[k, k - nx] = 1.0
        if j + 1 < ny:
            Jm[k, k + nx] = 1.0
        if family.endswith("_nl"):                       # + c^2 e
            e = x[k + 1] if i + 1 < nx else 0.0
            Jm[k, k] += 2.0 * x[k] * e
            if i + 1 < nx:
                Jm[k, k + 1] += x[k] ** 2
    return Jm


def true_residual(family, prm, x, alpha, beta, b, y):
    """||b - (alpha I + beta J_exact) y|| / ||b||."""
    A = alpha * np.eye(np.asarray(x).size) + beta * jacobian_dense(family, prm, x)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(b - A @ np.asarray(y, dtype=np.float64)) / np.linalg.norm(b))
