"""numpy restatement of the matrix-free trust-region consumer (csrc/fdjac_jftr.hip, fd_jftr_*): the Steihaug-Toint recurrence on the
finite-difference JVP, operation for operation, so that the device's y, r_out, exit, flags, iteration count and the four status scalars
can be compared BIT FOR BIT.  Not a test file: tests/test_jftr_model_cpu.py, tests/test_gpu_jftr.py and tests/jftr_switch_child.py use it.
It composes the existing models and has arithmetic of its own only where it cannot:

  the recurrence  cg() below: csc_tr_model.step copied word for word, with the product, the dot kappa = p.q and the three weighted dots
                  pi_pp, pi_yp, pi_yy of the direction update as callables (and m handed in).  With csc_tr_model's row product, dot_rows and
                  k_tr_p's dots plugged in it IS csc_tr_model.step, bit for bit: tests/test_jftr_model_cpu.py.
  the operator    q = lambda p + beta J(x) p is jfnk_model.operator (jvp_model's dot, epsilon and quotient; two multiplications and one
                  addition); kappa is csc_solve_model.dot_vec(p, q), a vector-kernel dot.
  the order       of dot(x, p), by jvp_enqueue's rule (jfnk_model.dot_order): "small" up to kSmallN; above it "paired" when x starts on a
                  pair (p is the consumer's own and always does), else "scalar".
  the pi dots     up to kSmallN (or with the fusion off): k_tr_p's, csc_solve_model.dot_vec.  Above it k_jt_p forms them in the traversal
                  of k_dot_partial on the JVP's grid: per thread in that kernel's element order, per workgroup by its shuffle tree and
                  red[] sum (wg_sums below restates jvp_model.dot_large's loop up to the workgroups' partials, the one piece that model
                  does not hand out), and then THE WORKGROUPS' SUMS IN ASCENDING INDEX from +0.0 -- not k_tr_p's order.
  the CU count    the large orders run on balanced_grid(ceil(N / 256), 8 num_cus) workgroups: a parameter, as in jvp_model."""
import numpy as np

import csc_solve_model as M
import csc_tr_model as TM
import jfnk_model as JM
import jvp_model as J

EXIT_INTERIOR, EXIT_BOUNDARY, EXIT_NEGATIVE, EXIT_UNBOUNDED = TM.EXIT_INTERIOR, TM.EXIT_BOUNDARY, TM.EXIT_NEGATIVE, TM.EXIT_UNBOUNDED
_not_finite = TM._not_finite


def cg(product, kappa_dot, pi_dots, m, m_bad, g, radius, rtol=1e-10, max_iterations=500, keep_unconverged=False, trace=None, log=None):
    """csc_tr_model.step with product(p) -> q, kappa_dot(p, q) and pi_dots(m, p, y) -> (pi_pp, pi_yp, pi_yy) as callables; m: the
    weights, m_bad: the start found one it cannot divide by.  Returns (y, r_out, status).  trace: a list that receives every iterate;
    log: a list that receives, per iteration, the numbers its decisions compared (kappa beside p.p; reach = ||y + alpha p||_W^2 against
    delta2 when kappa > 0; rho against tol2)."""
    with np.errstate(all="ignore"):
        g = np.asarray(g, dtype=np.float64)
        delta2 = np.float64(radius) * np.float64(radius)
        N = g.size
        flags, exit_kind = 0, 0
        if m_bad:
            flags |= 2
        r = g.copy()
        y = np.zeros(N)
        z = r / m
        p = -z
        gamma, rho0, ppp = M.dot_vec(r, z), M.dot_vec(r, r), M.dot_vec(m * p, p)
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
            q = product(p)
            kappa = kappa_dot(p, q)
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
                reach = pyy + 2.0 * alpha * pyp + alpha * alpha * ppp
                if reach >= delta2:
                    exit_kind, alpha = EXIT_BOUNDARY, tau
            y = y + alpha * p
            r = r + alpha * q
            z = r / m
            gamma_new, rho = M.dot_vec(r, z), M.dot_vec(r, r)
            iters += 1
            if trace is not None:
                trace.append(y.copy())
            if log is not None:
                log.append({"kappa": float(kappa), "pp": float(np.dot(p, p)), "reach": float(reach) if kappa > 0.0 else None, "delta2": float(delta2),
                            "rho": float(rho), "tol2": float(tol2), "exit": int(exit_kind)})
            if exit_kind != 0 or rho <= tol2:
                done = True
                break
            if _not_finite(gamma_new):
                flags |= 2
                break
            beta = gamma_new / gamma
            gamma = gamma_new
            p = -z + beta * p
            ppp, pyp, pyy = pi_dots(m, p, y)
        final = 2 if flags & 2 else (0 if done else 1)      # bit 1: breakdown; bit 0: the iterations ran out
        yw2 = M.dot_vec(m * y, y)
        pred = np.float64(-0.5) * M.dot_vec(y, g + r)
        if final and not keep_unconverged:
            y, r = np.full(N, np.nan), np.full(N, np.nan)
        return y, r, {"flags": int(final), "exit": int(exit_kind), "iterations": int(iters), "resid": float(np.sqrt(rho)),
                      "g_norm": float(np.sqrt(rho0)), "step_norm": float(np.sqrt(yw2)), "pred": float(pred)}


def pi_dots_vec(m, p, y):
    """k_tr_p's three dots."""
    return M.dot_vec(m * p, p), M.dot_vec(m * y, p), M.dot_vec(m * y, y)


def wg_sums(terms, paired, num_cus):
    """The workgroups' sums of `terms` in k_dot_partial<paired>'s traversal: jvp_model.dot_large up to its partials."""
    with np.errstate(all="ignore"):
        n = terms.size
        g = J.grid(n, num_cus)
        acc = np.zeros(g * J.BLOCK)
        if paired:
            n2 = n >> 1
            T = acc.size
            for r in range((n2 + T - 1) // T):            # a thread's pair: element .x, then element .y
                lo, hi = r * T, min((r + 1) * T, n2)
                acc[:hi - lo] = (acc[:hi - lo] + terms[2 * lo:2 * hi:2]) + terms[2 * lo + 1:2 * hi:2]
            if n & 1:                                      # the tail: thread 0 of block 0, after its own pairs
                acc[0] = acc[0] + terms[n - 1]
        else:
            acc = J._strided(acc, terms)
        return J._tree_waves(acc.reshape(g, J.BLOCK))


def ascending(parts):
    """From +0.0, the workgroups' sums in ascending index."""
    t = np.float64(0.0)
    with np.errstate(all="ignore"):
        for v in parts:
            t = t + v
    return t


def pi_dots_fused(m, p, y, paired, num_cus):
    """k_jt_p's three dots."""
    return tuple(ascending(wg_sums(t, paired, num_cus)) for t in ((m * p) * p, (m * y) * p, (m * y) * y))


def operator(f, x, v, lam, beta, fdtype="forward", x_aligned=True, v_aligned=True, small_off=False, num_cus=256, relstep=None, absstep=None,
             dir=1.0, f_in=None):
    """w = lam v + beta q as fd_jftr_apply_async computes it: q is fd_jvp_async's for (x, v)."""
    order = JM.dot_order(np.asarray(x).size, x_aligned, v_aligned, small_off)
    return JM.operator(f, x, v, lam, beta, fdtype, order, num_cus, relstep, absstep, dir, f_in)


def step(f, x, g, lam, beta, radius, fdtype="forward", m=None, rtol=1e-10, max_iterations=500, keep_unconverged=False, num_cus=256,
         relstep=None, absstep=None, dir=1.0, f_in=None, x_aligned=True, small_off=False, fuse=True, trace=None, counts=None, log=None):
    """min g.y + 1/2 y.(lam I + beta J(x)) y, ||y||_W <= radius, as fd_jftr_step_async computes it.  m: the caller's weights or None
    (W = I); x_aligned: whether the device array starts on a pair; small_off: FDJAC_SMALL=0; fuse: k_jt_p above kSmallN (False:
    FDJAC_JFTR_FUSE=0).  counts: a dict that receives "applications", the products the step used."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    napp = [0]
    order = JM.dot_order(N, x_aligned, True, small_off)

    def product(p):
        napp[0] += 1
        return JM.operator(f, x, p, lam, beta, fdtype, order, num_cus, relstep, absstep, dir, f_in)

    if m is None:
        mm, m_bad = np.ones(N), False
    else:
        mm = np.asarray(m, dtype=np.float64)
        with np.errstate(all="ignore"):
            m_bad = not np.all((mm > 0.0) & (mm < np.inf))
    if fuse and order != "small":
        pi = lambda w, p, y: pi_dots_fused(w, p, y, order == "paired", num_cus)          # noqa: E731
    else:
        pi = pi_dots_vec
    out = cg(product, M.dot_vec, pi, mm, m_bad, g, radius, rtol, max_iterations, keep_unconverged, trace, log)
    if counts is not None:
        counts["applications"] = napp[0]
    return out
