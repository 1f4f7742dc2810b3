"""Timing of the warm start of the sparse and the matrix-free consumer (fd_csc_solve_from_async / fd_jfnk_solve_from_async, DESIGN 4.9 and
4.12) in Float64: HIP events after a warm-up, the median with p10 - p90.  Three parts, written to profiles/warm_start.md down to its
"Annotations" heading (what stands below that heading there is written by hand):

  (a) the cold path did not slow down: fd_csc_solve_async (BiCGStab and GMRES, Jacobi, on the 5-point pattern at about 960 000 and
      8 000 000 unknowns) and fd_jfnk_solve_async (tridiagonal family, lazy quotient, 10^6 and 10^7) with a fixed number of iterations
      (rtol = 0), >= 30 solves after the warm-up.  Run it ONCE PER TREE in the same session on the same machine:
          python scripts/warm_start_probe.py --part a --root <parent checkout, built> --json parent.json
          python scripts/warm_start_probe.py --part a --json head.json
      and hand both to the report run (--cold-head head.json --cold-parent parent.json): the head's median must lie within the
      parent's own p10 - p90.  Part (a) uses nothing the parent tree lacks.
  (b) what the fused start costs: a warm solve capped at ONE iteration minus a cold solve capped at one iteration (the two differ in
      the start alone: k_cs_init_from for k_cs_init; the operator application and k_jf_from for nothing), against one cold iteration
      (a solve capped at 11 minus one capped at 1, over 10), at about 8 000 000 unknowns.
  (c) warm against cold: iterations and time to solution over 10 steps of (I - gamma J) u+ = u on the 2000 x 2000 5-point pattern,
      cold and from y0 = b, for the homogeneous Laplacian and for the heterogeneous coefficient of tests/warm_cases.py scaled to the grid.

    python scripts/warm_start_probe.py --head $(git rev-parse --short=12 HEAD) [--part abc] [--reps 30] [--cold-head F --cold-parent F]"""
import argparse
import json
import os
import sys

import numpy as np

GAMMA = 0.1


def timed(torch, fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts = np.sort(np.array(ts))
    return float(np.median(ts)), float(ts[int(0.1 * (len(ts) - 1))]), float(ts[int(round(0.9 * (len(ts) - 1)))])


def lap5(P, torch, nx, ny, coef=None):
    """(colptr, rowval 1-based, nz on the device) of diag(coef) * the 5-point Laplacian."""
    colptr, rowval = P.lap5_csc(nx, ny)
    cols = P.csc_cols(colptr)
    nz = np.where(rowval == cols, -4.0, 1.0)
    if coef is not None:
        nz = nz * coef[rowval - 1]
    return colptr, rowval, torch.as_tensor(nz, device="cuda")


def part_a(fd, P, torch, reps):
    out = {}
    for nx, ny in ((980, 980), (2828, 2829)):
        N = nx * ny
        colptr, rowval, nz = lap5(P, torch, nx, ny)
        b = torch.as_tensor(np.random.default_rng(N).uniform(-1.0, 1.0, N), device="cuda")
        y = torch.empty_like(b)
        s = fd.CscSolver((colptr, rowval, N), idx_base=1)
        for method, its in (("bicgstab", 8), ("gmres", 8)):
            s.set_method(method, 8)
            s.set_options(0.0, its)
            s.set_policy(True)
            out["csc %s N=%d %d iterations" % (method, N, its)] = timed(torch, lambda: s.solve(nz, b, y, 1.0, -GAMMA), reps)
            assert s.status()["iterations"] == its
        del s
    for N in (1000000, 10000000):
        rng = np.random.default_rng(N)
        x = torch.as_tensor(rng.random(N) - 0.25, device="cuda")
        b = torch.as_tensor(rng.uniform(-1.0, 1.0, N), device="cuda")
        y = torch.empty_like(b)
        f = fd.BuiltinF("tridiag", N)
        s = fd.JfnkSolver(N, "forward", 8)
        s.set_lazy(f)
        s.set_options(0.0, 8)
        s.set_policy(True)
        out["jfnk lazy quotient N=%d 8 iterations" % N] = timed(torch, lambda: s.solve(f, x, b, y, 1.0, -0.3), reps)
        assert s.status()["iterations"] == 8
        del s, f
        torch.cuda.empty_cache()
    return out


def part_b(fd, P, torch, reps, lines):
    nx, ny = 2828, 2829
    N = nx * ny
    colptr, rowval, nz = lap5(P, torch, nx, ny)
    rng = np.random.default_rng(7)
    b = torch.as_tensor(rng.uniform(-1.0, 1.0, N), device="cuda")
    y0 = torch.as_tensor(rng.uniform(-1.0, 1.0, N), device="cuda")
    y = torch.empty_like(b)
    lines += ["## (b) the fused start against one cold iteration, N = %d" % N, "",
              "| solver | cold, 1 iteration, us | warm, 1 iteration, us | the start's extra cost, us | one cold iteration, us | start / iteration |", "|---|---|---|---|---|---|"]
    s = fd.CscSolver((colptr, rowval, N), idx_base=1)
    s.set_policy(True)
    rows = []
    for method in ("bicgstab", "gmres"):
        s.set_method(method, 30)
        s.set_options(0.0, 1)
        c1 = timed(torch, lambda: s.solve(nz, b, y, 1.0, -GAMMA), reps)
        w1 = timed(torch, lambda: s.solve(nz, b, y, 1.0, -GAMMA, y0=y0), reps)
        s.set_options(0.0, 11)
        c11 = timed(torch, lambda: s.solve(nz, b, y, 1.0, -GAMMA), reps)
        rows.append(("sparse, %s, Jacobi" % method, c1, w1, c11))
    del s
    x = torch.as_tensor(rng.random(N) - 0.25, device="cuda")
    f = fd.BuiltinF("tridiag", N)
    j = fd.JfnkSolver(N, "forward", 30)
    j.set_lazy(f)
    j.set_policy(True)
    j.set_options(0.0, 1)
    c1 = timed(torch, lambda: j.solve(f, x, b, y, 1.0, -0.3), reps)
    w1 = timed(torch, lambda: j.solve(f, x, b, y, 1.0, -0.3, y0=y0), reps)
    j.set_options(0.0, 11)
    c11 = timed(torch, lambda: j.solve(f, x, b, y, 1.0, -0.3), reps)
    rows.append(("matrix-free, tridiagonal family, lazy quotient", c1, w1, c11))
    for name, c1, w1, c11 in rows:
        it = (c11[0] - c1[0]) / 10.0
        lines.append("| %s | %.0f (%.0f - %.0f) | %.0f (%.0f - %.0f) | %.0f | %.0f | %.2f |" % ((name,) + c1 + w1 + (w1[0] - c1[0], it, (w1[0] - c1[0]) / it)))
    lines.append("")


def part_c(fd, P, torch, lines):
    nx = ny = 2000
    N = nx * ny
    k = np.arange(N)
    i, jj = k % nx, k // nx
    rough = np.random.default_rng(12).uniform(-1.0, 1.0, N)
    corner = (i < nx // 2) & (jj < ny // 2)
    rim = (i < nx // 2 + 1) & (jj < ny // 2 + 1)
    cases = (("homogeneous Laplacian, gamma = 1", None, 1.0, rough),
             ("c = 1 in a quarter of the grid, 1e-4 elsewhere; the state starts outside it; gamma = 100", np.where(corner, 1.0, 1e-4), 100.0, np.where(rim, 0.0, rough)))
    lines += ["## (c) warm (y0 = b) against cold over 10 steps of (I - gamma J) u+ = u, 2000 x 2000, BiCGStab, Jacobi, rtol 1e-10", "",
              "| case | cold iterations per step | warm iterations per step | cold, us (10 steps) | warm, us (10 steps) |", "|---|---|---|---|---|"]
    for name, coef, gamma, u0 in cases:
        colptr, rowval, nz = lap5(P, torch, nx, ny, coef)
        s = fd.CscSolver((colptr, rowval, N), idx_base=1)
        s.set_options(1e-10, 2000)
        res = {}
        for warm in (False, True):
            u = torch.as_tensor(u0, device="cuda")
            y = torch.empty_like(u)
            its, total = [], 0.0
            for _step in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                s.solve(nz, u, y, 1.0, -gamma, y0=u if warm else None)
                e1.record(); e1.synchronize()
                st = s.status()
                its.append(st["iterations"] if st["flags"] == 0 else "%d (flags %d)" % (st["iterations"], st["flags"]))
                total += e0.elapsed_time(e1) * 1e3
                u, y = y, u
            res[warm] = (its, total)
        lines.append("| %s | %s | %s | %.0f | %.0f |" % (name, res[False][0], res[True][0], res[False][1], res[True][1]))
        del s
        torch.cuda.empty_cache()
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default="unknown")
    ap.add_argument("--part", default="abc")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package is measured")
    ap.add_argument("--json", default=None, help="part (a) alone: write its figures here and no report")
    ap.add_argument("--cold-head", default=None)
    ap.add_argument("--cold-parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    import finitediff_jl_amd as fd
    from finitediff_jl_amd import patterns as P
    assert os.path.abspath(fd.__file__).startswith(os.path.abspath(a.root)), fd.__file__
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(part_a(fd, P, torch, a.reps), fh, indent=1)
        return
    lines = ["# Warm start of the sparse and the matrix-free consumer (Float64)", "",
             "`scripts/warm_start_probe.py` at %s on %s.  Times in microseconds between HIP events: median (p10 - p90) of %d solves after 5 warm-up solves."
             % (a.head, torch.cuda.get_device_name(0), a.reps), ""]
    if "a" in a.part:
        head = json.load(open(a.cold_head)) if a.cold_head else part_a(fd, P, torch, a.reps)
        parent = json.load(open(a.cold_parent)) if a.cold_parent else None
        lines += ["## (a) the cold path (y0 = NULL) against the parent commit, one session, one machine", "",
                  "| solve | parent, us | this commit, us | inside the parent's p10 - p90 |", "|---|---|---|---|"]
        for key, h in head.items():
            p = parent.get(key) if parent else None
            lines.append("| %s | %s | %.0f (%.0f - %.0f) | %s |" % (key, "%.0f (%.0f - %.0f)" % tuple(p) if p else "not measured", h[0], h[1], h[2],
                                                                   ("yes" if p[1] <= h[0] <= p[2] else "NO") if p else "-"))
        lines.append("")
    if "b" in a.part:
        part_b(fd, P, torch, a.reps, lines)
    if "c" in a.part:
        part_c(fd, P, torch, lines)
    lines += ["## Annotations (by hand, not by the script)", ""]
    out = a.out or os.path.join(a.root, "profiles", "warm_start.md")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
