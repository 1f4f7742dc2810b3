"""Timing of the matrix-free trust-region consumer (fd_jftr_step_async) in Float64 on the tridiagonal built-in family:
B = 1/2 I - J, W = I, no boundary, rtol = 0 and max_iterations = ITERS, so that every step runs exactly ITERS iterations.  HIP events
around one step, 10 warm-up steps, then 50 samples: the median with min - p90, divided by ITERS (the start kernel, the end kernel, the
base evaluation and two record read-backs are inside: 3 launches per step beside ITERS times the iteration's).  Three rows per size:
    JfTrustRegion on the lazy-quotient route (k_jt_p above kSmallN);
    the same with k_jt_p's fusion switched off (FDJAC_JFTR_FUSE=0: k_tr_p, then the JVP's own k_dot_partial);
    CscTrustRegion on the stored tridiagonal H = -J of the same system (lambda = 1/2).
The fusion switch is a test switch: the script sets FDJAC_TEST_SWITCHES=1 for itself.  Writes profiles/jftr.md down to its
"Annotations" heading; what stands below that heading there is written by hand.

    python scripts/jftr_probe.py --head $(git rev-parse --short=12 HEAD) [--sizes 1000000,10000000] [--iters 24]"""
import argparse
import os
import sys

os.environ["FDJAC_TEST_SWITCHES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                             # noqa: E402
import torch                                   # noqa: E402
import finitediff_jl_amd as fd                 # noqa: E402
from finitediff_jl_amd import patterns as P    # noqa: E402

LAM, BETA = 0.5, -1.0
LAUNCHES = {"fused": "5: k_jvp_eps, f!, k_jt_close, k_tr_update, k_jt_p", "unfused": "6: k_dot_partial, k_jvp_eps, f!, k_jt_close, k_tr_update, k_tr_p",
            "stored": "3: k_tr_rows, k_tr_update, k_tr_p"}


def timed(fn, reps, warm):
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
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jftr.md"))
    a = ap.parse_args()
    K = a.iters
    lines = ["# Matrix-free trust-region consumer: time per Steihaug-Toint iteration (Float64, tridiagonal family)", "",
             "`scripts/jftr_probe.py` at %s on %s.  One step = %d iterations (rtol = 0, max_iterations = %d, no boundary, W = I), its start, its end"
             % (a.head, torch.cuda.get_device_name(0), K, K),
             "and one base evaluation; median (min - p90) of %d steps between HIP events after %d warm-up steps; per iteration = step / %d."
             % (a.reps, a.warm, K), "Launches per iteration: derived from the schedule (DESIGN 4.13), not counted from a trace.", "",
             "| N | consumer | step, us | per iteration, us | launches per iteration |", "|---|---|---|---|---|"]
    for N in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(N)
        x = torch.as_tensor(rng.random(N) - 0.25, device="cuda")
        g = torch.as_tensor(rng.uniform(-1.0, 1.0, N), device="cuda")
        y = torch.empty(N, dtype=torch.float64, device="cuda")
        f = fd.BuiltinF("tridiag", N)
        row = {}
        for name, fuse in (("fused", "1"), ("unfused", "0")):
            os.environ["FDJAC_JFTR_FUSE"] = fuse          # (read at creation)
            s = fd.JfTrustRegion(N, "forward")
            s.set_lazy(f, quotient=True)
            s.set_options(0.0, K)
            s.set_policy(True)
            row[name] = timed(lambda: s.step(f, x, g, y, float("inf"), LAM, BETA), a.reps, a.warm)
            st = s.status()
            assert st["iterations"] == K and st["flags"] == 1, st
            label = "JfTrustRegion, lazy quotient" + ("" if name == "fused" else ", FDJAC_JFTR_FUSE=0 (k_tr_p + the JVP's own dot)")
            lines.append("| %d | %s | %.0f (%.0f - %.0f) | %.1f | %s |" % ((N, label) + row[name] + (row[name][0] / K, LAUNCHES[name])))
            del s
        os.environ["FDJAC_JFTR_FUSE"] = "1"
        # the stored route: H = -J of the same system in CSC storage, lambda = 1/2
        colptr, rowval = P.tridiag_csc(N)
        base = int(colptr[0])
        cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
        nz = torch.as_tensor(np.where(rowval - base == cols, 2.0, -1.0), device="cuda")
        H = fd.SparseMatrixCSC(N, N, colptr, rowval, nz)
        cs = fd.CscTrustRegion(H)
        cs.set_options(0.0, K)
        cs.set_policy(True)
        row["stored"] = timed(lambda: cs.step(nz, g, y, float("inf"), LAM, "I"), a.reps, a.warm)
        st = cs.status()
        assert st["iterations"] == K and st["flags"] == 1, st
        lines.append("| %d | CscTrustRegion, stored tridiagonal H | %.0f (%.0f - %.0f) | %.1f | %s |"
                     % ((N,) + row["stored"] + (row["stored"][0] / K, LAUNCHES["stored"])))
        lines.append("| %d | fused / unfused direction update | %.3f | | |" % (N, row["fused"][0] / row["unfused"][0]))
        del cs, H, nz
        torch.cuda.empty_cache()
    lines += ["", "## Annotations (by hand, not by the script)", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
