"""Timing of the block ILU(0) preconditioner of the sparse consumer (fd_csc_solver_set_block_ilu) in Float64 beside the
diagonal one of the same case in the same process: HIP events, 10 warm-up and 50 timed solves, the median with min - p90.  Cases: the
5-point Laplacian on 1000 x 1000 points with A = I - 10 J, and the random band of scripts/csc_solver_probe.py (2e6 columns, 6 entries per
column within +-300, gamma max||row||_1 = 0.9).  Block sizes 256 and 1024.  Writes profiles/csc_ilu.md.

The yardstick is the diagonal-preconditioned solve: that code does not change with this preconditioner.

The fixed part of a solve.  With b = 0 and max_iterations = 1 a solve is its fixed part: the start kernel (which finds ||b|| = 0 and sets
`done`), with block ILU the factor kernel (it does not look at `done`), ONE iteration's kernels, which leave at once, one record and the
final kernel.  "factor us" is the DIFFERENCE of the two fixed parts (medians): k_cs_ilu_factor plus two applies that leave at once, minus
the diagonal that only the Jacobi start kernel forms.  "us / iteration" is (solve - fixed part) / iterations.

    python scripts/csc_ilu_probe.py --head $(git rev-parse --short=12 HEAD) [--small]
The script itself does not touch the GPU: every case runs in a child process of its own under a time limit, one after the other, and the
first child that fails ends the run."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (256, 1024)
CHILD_LIMIT = 420          # seconds per case
T0 = time.time()


def note(*what):
    print("[%6.1f s]" % (time.time() - T0), *what, file=sys.stderr, flush=True)


def timed(torch, np, fn, reps=50, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts = np.sort(np.array(ts))
    return [float(np.median(ts)), float(ts[0]), float(ts[int(0.9 * (len(ts) - 1))])]


def child(case, small):
    """One case: the diagonal, then block ILU at every size, on one solver.  Prints one JSON line."""
    import numpy as np
    import torch
    import finitediff_jl_amd as fd
    import csc_solve_model as M
    import test_cscilu_model_cpu as H
    from csc_solver_probe import band_pattern
    ctx = fd.Context.default()
    gb = C.c_double()
    fd.lib.check(ctx.L.fd_stream_copy_gbps(ctx.handle, 1 << 28, 10, C.byref(gb)))
    if case == "lap5":
        n = 100 if small else 1000
        colptr, rowval, N = M.lap5_pattern(n, n)
        nz = torch.as_tensor(H.stencil_values(n, n, (1.0, -2.0, 1.0), (1.0, -2.0, 1.0)), device="cuda")
        gamma, title = 10.0, "5-point %d x %d, A = I - 10 J" % (n, n)
    else:
        colptr, rowval, N = band_pattern(20000 if small else 2 * 10 ** 6, 300, 6, 11)
        g = torch.Generator(device="cuda"); g.manual_seed(3)
        nz = torch.rand(rowval.size, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
        rowsum = torch.zeros(N, dtype=torch.float64, device="cuda").index_add_(0, torch.as_tensor(rowval, device="cuda"), nz.abs())
        gamma, title = 0.9 / float(rowsum.max()), "random band %d x 6 (+-300), gamma max||row||_1 = 0.9" % N
    note(title, "N = %d nnz = %d" % (N, rowval.size))
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    b = torch.randn(N, generator=g, device="cuda", dtype=torch.float64)
    zero = torch.zeros(N, dtype=torch.float64, device="cuda")
    y = torch.empty(N, dtype=torch.float64, device="cuda")
    s = fd.CscSolver((torch.as_tensor(colptr.astype(np.int32), device="cuda"), torch.as_tensor(rowval.astype(np.int32), device="cuda"), N), idx_base=0)
    rows = []
    for bs in (0,) + SIZES:
        t_set = time.time()
        if bs:
            s.set_block_ilu(bs)
        else:
            s.set_preconditioner("jacobi")
        t_set = time.time() - t_set
        s.set_options(1e-10, 500)
        s.solve(nz, b, y, 1.0, -gamma)
        st = s.status()
        levels = list(s.ilu_levels()[2:]) if bs else [0, 0]
        note(title, "bs", bs, st, "levels", levels)
        t = timed(torch, np, lambda: s.solve(nz, b, y, 1.0, -gamma))
        s.set_options(1e-10, 1)
        t0 = timed(torch, np, lambda: s.solve(nz, zero, y, 1.0, -gamma))
        st0 = s.status()
        assert st0["flags"] == 0 and st0["iterations"] == 0, st0
        rows.append({"bs": bs, "flags": st["flags"], "iterations": st["iterations"], "solve": t, "fixed": t0, "levels": levels, "schedule_s": t_set})
    print(json.dumps({"title": title, "N": N, "nnz": int(rowval.size), "gbps": gb.value, "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("lap5", "band"), default=None)
    ap.add_argument("--head", default="unknown")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csc_ilu.md"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.small)
    results = []
    for case in ("lap5", "band"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case] + (["--small"] if a.small else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)      # (its progress goes to this process's stderr)
        if r.returncode != 0:
            print("case %s failed (exit %d): nothing further is started" % (case, r.returncode), file=sys.stderr)
            return r.returncode or 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    lines = ["# Sparse consumer: block ILU(0) against Jacobi preconditioning (Float64)", "", "head: %s" % a.head, "",
             "Times in microseconds: median (min - p90) of 50 HIP-event samples after 10 warm-up solves; rtol 1e-10.  Every case in a process of its "
             "own, with the stream-copy ceiling (`fd_stream_copy_gbps`) measured in that process.  Fixed part: the same solve with b = 0 and "
             "max_iterations = 1.  factor us = fixed part with block ILU - fixed part with the diagonal.  us / iteration = (solve - fixed part) / "
             "iterations.  Levels: the largest forward + backward level count of a block (a barrier each, per apply).  The yardstick is the "
             "diagonal-preconditioned solve of the same case in the same process.", "",
             "| case | N | ceiling GB/s | preconditioner | levels fwd + bwd | iterations (flags) | solve us | fixed part us | factor us | us / iteration | solve / diagonal solve |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    verdict = []
    for res in results:
        base = res["rows"][0]
        for r in res["rows"]:
            kind = "block ILU(0), bs = %d" % r["bs"] if r["bs"] else "diagonal"
            lines.append("| %s | %d | %.0f | %s | %s | %d (%d) | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %s | %.1f | %.2f |" % (
                res["title"], res["N"], res["gbps"], kind, "%d + %d" % (r["levels"][0] + 1, r["levels"][1] + 1) if r["bs"] else "-",
                r["iterations"], r["flags"], *r["solve"], *r["fixed"], "%.1f" % (r["fixed"][0] - base["fixed"][0]) if r["bs"] else "-",
                (r["solve"][0] - r["fixed"][0]) / max(1, r["iterations"]), r["solve"][0] / base["solve"][0]))
            if r["bs"]:
                # shorter or longer only when the min - p90 ranges do not overlap
                word = "SHORTER than" if r["solve"][2] < base["solve"][1] else ("LONGER than" if r["solve"][1] > base["solve"][2] else "not distinguishable from")
                verdict.append("- %s, bs = %d: %d iterations against %d; time to solution is %s the diagonal's (%.2f x)." % (
                    res["title"], r["bs"], r["iterations"], base["iterations"], word, r["solve"][0] / base["solve"][0]))
    lines += ["", "## In plain words", ""] + verdict
    lines += ["", "The schedule is built on the host when the preconditioner is selected (not on the hot path): " +
              "; ".join("%s: %s" % (res["title"], ", ".join("bs %d %.2f s" % (r["bs"], r["schedule_s"]) for r in res["rows"] if r["bs"])) for res in results) + "."]
    text = "\n".join(lines) + "\n"
    print(text)
    if not a.no_write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
