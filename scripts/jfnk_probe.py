"""Timing of the matrix-free consumer (fd_jfnk_solve_async) in Float64 on the tridiagonal built-in family: HIP events after
a warm-up, the median with min - p90 of a solve capped at ONE cycle of `restart` Arnoldi steps (rtol = 0, so every step runs), divided by
the steps: time per GMRES step on the plain, lazy-values and lazy-quotient routes, with and without a diagonal.  Beside it the stored
route on the same system: the coloured Jacobian (three colours, the family's storing launch) and fd_csc_solve_async with GMRES capped
the same way.  The launches per step are those of DESIGN 4.12's table (derived from the schedule, not counted from a trace).
Writes profiles/jfnk.md down to its "Annotations" heading; what stands below that heading there is written by hand.

    python scripts/jfnk_probe.py --head $(git rev-parse --short=12 HEAD) [--sizes 1000000,10000000] [--restart 30] [--reps 7]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P

GAMMA = 0.3
LAUNCHES = {"plain": 8 + 5, "lazy": 8 + 4, "quot": 8 + 4, "stored": 10}


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts = np.sort(np.array(ts))
    return float(np.median(ts)), float(ts[0]), float(ts[min(len(ts) - 1, int(0.9 * len(ts)))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default="unknown")
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jfnk.md"))
    a = ap.parse_args()
    m = a.restart
    lines = ["# Matrix-free consumer: time per GMRES step (Float64, tridiagonal family, restart %d)" % m, "",
             "`scripts/jfnk_probe.py` at %s on %s.  One solve = one cycle of %d steps and its end (rtol = 0, max_iterations = %d), median (min - p90)"
             % (a.head, torch.cuda.get_device_name(0), m, m),
             "of %d solves between HIP events after 2 warm-up solves; per step = solve / %d.  Launches per step: derived from the schedule." % (a.reps, m), "",
             "| N | route | diagonal | solve, us | per step, us | launches per step |", "|---|---|---|---|---|---|"]
    for N in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(N)
        x = torch.as_tensor(rng.random(N) - 0.25, device="cuda")
        b = torch.as_tensor(rng.uniform(-1.0, 1.0, N), device="cuda")
        d = torch.full((N,), 1.0 + 2.0 * GAMMA, dtype=torch.float64, device="cuda")
        y = torch.empty(N, dtype=torch.float64, device="cuda")
        f = fd.BuiltinF("tridiag", N)
        for route in ("plain", "lazy", "quot"):
            for diag in (False, True):
                s = fd.JfnkSolver(N, "forward", m)
                s.set_lazy(f if route != "plain" else None, quotient=route == "quot")
                s.set_options(0.0, m)
                s.set_policy(True)
                s.set_diagonal(d if diag else None)
                med, lo, p90 = timed(lambda: s.solve(f, x, b, y, 1.0, -GAMMA), a.reps)
                assert s.status()["iterations"] == m
                lines.append("| %d | %s | %s | %.0f (%.0f - %.0f) | %.1f | %d |" % (N, route, "yes" if diag else "no", med, lo, p90, med / m, LAUNCHES[route]))
                del s
        # the stored route: the coloured Jacobian, then GMRES on its nzval
        colptr, rowval = P.tridiag_csc(N)
        colors = P.cyclic_colors(N, 3)
        J = fd.SparseMatrixCSC(N, N, colptr, rowval, torch.zeros(rowval.size, dtype=torch.float64, device="cuda"))
        cache = fd.JacobianCache(x, fdtype="forward", colorvec=colors, sparsity=J)
        jac = timed(lambda: fd.finite_difference_jacobian_b(J, f, x, cache), a.reps)
        cs = fd.CscSolver(J)
        cs.set_method("gmres", m)
        cs.set_options(0.0, m)
        cs.set_policy(True)
        med, lo, p90 = timed(lambda: cs.solve(J, b, y, 1.0, -GAMMA), a.reps)
        assert cs.status()["iterations"] == m
        lines.append("| %d | stored: coloured Jacobian (drop-in call through its cache, plan lookup included) | - | %.0f (%.0f - %.0f) | - | - |" % ((N,) + jac))
        lines.append("| %d | stored: fd_csc_solve_async, GMRES | Jacobi | %.0f (%.0f - %.0f) | %.1f | %d |" % (N, med, lo, p90, med / m, LAUNCHES["stored"]))
        del cs, cache, J
        torch.cuda.empty_cache()
    lines += ["", "## Annotations (by hand, not by the script)", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
