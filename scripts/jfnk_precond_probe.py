"""Iterations and time to solution of the matrix-free consumer (fd_jfnk_solve_async) with a LAGGED stored Jacobian as its
right preconditioner (fd_jfnk_solver_set_csc_preconditioner), in Float64 on the nonlinear 5-point family near N = 10^6: the same system
(I - gamma J(x)) y = b with no preconditioner, with the diagonal, with block Jacobi 32 and with block ILU(0) 1024.  A JacobianCache
stores J(x0) once; each kind is factored once from it (fd_csc_solver_factor_async) and serves the solve at x0 and the solve at a
perturbed x1 = x0 + 0.05 u.  Time to solution: wall clock of the solve call and the status read that synchronises it (a solve waits for
its own records, so HIP events around it measure the same), median (min - p90) after a warm-up.  A record, not a gate.
Writes its table to --out (default profiles/jfnk_precond_table.md); profiles/jfnk_precond.md holds a run of it, pasted by hand beside
the step counts of the suites and the annotations.

    python scripts/jfnk_precond_probe.py --head $(git rev-parse --short=12 HEAD) [--grid 1000,1000] [--gamma 0.3] [--rtol 1e-6] [--reps 5]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P

KINDS = (("none", None), ("diagonal", ("jacobi",)), ("block Jacobi 32", ("block", 32)), ("block ILU(0) 1024", ("ilu", 1024)))


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.sort(np.array(ts))
    return float(np.median(ts)), float(ts[0]), float(ts[min(len(ts) - 1, int(0.9 * len(ts)))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default="unknown")
    ap.add_argument("--grid", default="1000,1000")
    ap.add_argument("--gamma", type=float, default=0.3)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jfnk_precond_table.md"))
    a = ap.parse_args()
    nx, ny = (int(s) for s in a.grid.split(","))
    N = nx * ny
    rng = np.random.default_rng(N)
    x0 = torch.as_tensor(rng.random(N) - 0.25, device="cuda")
    x1 = x0 + 0.05 * torch.as_tensor(rng.random(N), device="cuda")
    b = torch.as_tensor(rng.uniform(-1.0, 1.0, N), device="cuda")
    y = torch.empty(N, dtype=torch.float64, device="cuda")
    f = fd.BuiltinF("lap5_nl", nx, ny)
    colptr, rowval = P.lap5_csc(nx, ny)
    J = fd.SparseMatrixCSC(N, N, colptr, rowval, torch.zeros(rowval.size, dtype=torch.float64, device="cuda"))
    cache = fd.JacobianCache(x0, fdtype="forward", colorvec=P.lap5_colors(nx, ny), sparsity=J)
    fd.finite_difference_jacobian_b(J, f, x0, cache)          # J(x0), stored once
    lines = ["# Matrix-free consumer preconditioned by a lagged stored Jacobian (Float64, lap5_nl %d x %d, N = %d)" % (nx, ny, N), "",
             "`scripts/jfnk_precond_probe.py` at %s on %s.  (I - %g J(x)) y = b, forward differences, the lazy quotient route, GMRES(%d), rtol = %g,"
             % (a.head, torch.cuda.get_device_name(0), a.gamma, a.restart, a.rtol),
             "max_iterations = 500.  J(x0) is stored once by a JacobianCache; every kind is factored ONCE from it (`factor`, ms: one call and its",
             "status read) and serves both solves: at x0 and at x1 = x0 + 0.05 u.  Time to solution: wall clock of `solve` + `status`, median",
             "(min - p90) of %d after one warm-up." % a.reps, "",
             "| preconditioner | factor, ms | x0: flags | x0: steps | x0: ms | x1: flags | x1: steps | x1: ms |", "|---|---|---|---|---|---|---|---|"]
    for name, kind in KINDS:
        s = fd.JfnkSolver(N, "forward", a.restart)
        s.set_lazy(f, quotient=True)
        s.set_options(a.rtol, 500)
        s.set_policy(True)
        fac = "-"
        pc = None
        if kind is not None:
            pc = fd.CscSolver(J)
            if kind[0] == "jacobi":
                pc.set_preconditioner("jacobi")
            elif kind[0] == "block":
                pc.set_preconditioner("block_jacobi", kind[1])
            else:
                pc.set_block_ilu(kind[1])

            def factor():
                pc.factor(J, 1.0, -a.gamma)
                assert pc.factor_status()["flags"] == 0

            fac = "%.2f (%.2f - %.2f)" % timed(factor, a.reps)
            s.set_preconditioner(pc)
        cells = []
        for x in (x0, x1):
            def solve():
                s.solve(f, x, b, y, 1.0, -a.gamma)
                return s.status()

            med, lo, p90 = timed(solve, a.reps)
            st = solve()
            cells += [str(st["flags"]), str(st["iterations"]), "%.2f (%.2f - %.2f)" % (med, lo, p90)]
        lines.append("| %s | %s | %s |" % (name, fac, " | ".join(cells)))
        del s, pc
        torch.cuda.empty_cache()
    lines += ["", "## Annotations (by hand, not by the script)", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
