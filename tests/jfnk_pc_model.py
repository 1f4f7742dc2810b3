"""numpy restatement of the matrix-free consumer preconditioned by a LAGGED STORED JACOBIAN (fd_jfnk_solver_set_csc_preconditioner:
csrc/fdjac_jfnk.hip on a factorisation of csrc/fdjac_cscsolve.hip's fd_csc_solver_factor_async).  No arithmetic of its own: the cycle
is jfnk_model.gmres, the operator jfnk_model.operator, the factorisation and its application csc_gmres_model.preconditioner -- that is
csc_block_model.block_inverses / apply_planes, csc_ilu_model.factor / apply, or the division by the modelled diagonal -- and pre_bad is
the factorisation's.  Not a test file: tests/test_jfnk_pc_model_cpu.py, tests/test_gpu_csc_factor.py and tests/test_gpu_jfnk_pc.py use it.

  lag      the factorisation is built ONCE from (alpha0, beta0, nz0) -- J stored at some x0 -- and reused at the solve's x, alpha, beta.
  order    z of every step is the solver's own vector (always on a pair), so dot(x, z) runs in
           jfnk_model.dot_order(N, x_aligned, True, small_off) for every step and for the explicit residual.
FAULTS (deliberately wrong variants, for the tests of the tests):
  "factor_at_x1"       the factorisation is rebuilt from (alpha, beta, nz_now) of the solve instead of the lagged one
  "end_without_apply"  the cycle's end adds u instead of M^-1 u
  "fma_apply"          the block apply with a fused multiply-add (emulated in extended precision, rounded once per term)"""
import numpy as np

import csc_block_model as BM
import csc_gmres_model as G
import jfnk_model as JM

FAULTS = (None, "factor_at_x1", "end_without_apply", "fma_apply")


def factorisation(rl, alpha0, beta0, nz0, precond):
    """-> (apply(v) -> M^-1 v, bad) for precond ("jacobi",) | ("block", bs) | ("ilu", bs): csc_gmres_model.preconditioner as it is."""
    with np.errstate(all="ignore"):
        return G.preconditioner(rl, np.float64(alpha0), np.float64(beta0), np.asarray(nz0, dtype=np.float64), precond)


def _fma_planes(planes, x):
    """csc_block_model.apply_planes with acc = fma(plane, x, acc): the product is kept in extended precision and rounded with the sum."""
    bs, N = planes.shape
    i = np.arange(N)
    b0 = i // bs * bs
    n = np.minimum(bs, N - b0)
    acc = np.zeros(N)
    with np.errstate(all="ignore"):
        for c in range(bs):
            on = n > c
            acc[on] = (acc[on].astype(np.longdouble) + planes[c, on].astype(np.longdouble) * x[b0[on] + c].astype(np.longdouble)).astype(np.float64)
    return acc


def solve(f, x, b, alpha, beta, rl, lagged, precond, fdtype="forward", rtol=1e-10, max_iterations=500, keep_unconverged=False, restart=30,
          num_cus=256, relstep=None, absstep=None, dir=1.0, f_in=None, x_aligned=True, small_off=False, fault=None, trace=None, nz_now=None):
    """(alpha I + beta J(x)) y = b as fd_jfnk_solve_async computes it with a csc preconditioner set.  rl: csc_solve_model.RowLists of
    the stored pattern; lagged = (alpha0, beta0, nz0): what fd_csc_solver_factor_async was given; precond: the kind selected on the
    lent handle.  nz_now: J's stored values at the solve's x ("factor_at_x1" alone reads them).  trace also receives "applications"."""
    assert fault in FAULTS
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    a0, b0, nz0 = lagged
    if fault == "factor_at_x1":
        a0, b0, nz0 = alpha, beta, nz_now
    apply, pre_bad = factorisation(rl, a0, b0, nz0, precond)
    if fault == "fma_apply" and precond[0] == "block":
        planes, _bad = BM.block_inverses(rl.colptr, rl.rowval, N, np.float64(a0), np.float64(b0), np.asarray(nz0, dtype=np.float64), int(precond[1]))
        apply = lambda v: _fma_planes(planes, v)          # noqa: E731
    if fault == "end_without_apply":
        # jfnk_model.gmres hands apply() the basis rows themselves (views of V) at a step and a freshly summed u at a cycle's end
        step_apply = apply
        apply = lambda v: step_apply(v) if v.base is not None else np.array(v, dtype=np.float64)          # noqa: E731
    order = JM.dot_order(N, x_aligned, True, small_off)
    napp = [0]

    def product(v, kind, j):
        napp[0] += 1
        return JM.operator(f, x, v, alpha, beta, fdtype, order, num_cus, relstep, absstep, dir, f_in)

    y, st = JM.gmres(product, apply, pre_bad, b, rtol, max_iterations, keep_unconverged, restart, None, trace)
    if trace is not None:
        trace["applications"] = napp[0]
    return y, st
