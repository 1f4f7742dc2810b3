"""Time of the pivoted tridiagonal solve beside the default one, on one diagonally dominant system (both paths solve it), at
N = 10^6 and 10^7, both layouts: HIP events around each solve on the context's stream, warm-up first, the median of repeated runs, one
quiet process (nothing else on the GPU while it runs).  Writes profiles/tripivot.md.

    python scripts/tripivot_probe.py --head $(git rev-parse --short=12 HEAD) [--small]

Byte model of the pivoted solve (not a claim of speed): level 0 reads 4 N values twice and writes N; every further level is a quarter
of the one below with 4 values in, 4 out and 1 solution value per row, written and read once each: about 13 N doubles, 1.04 GB at
N = 10^7, no less than 0.13 ms at 8 TB/s."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import finitediff_jl_amd as fd      # noqa: E402
import tri_pivot_model as M         # noqa: E402


def csc_nzval(dl, d, du):
    N = d.size
    out = np.empty(3 * N - 2, d.dtype)
    j = np.arange(N)
    out[np.where(j > 0, 3 * j, 0)] = d
    out[3 * j[1:] - 1] = du
    out[3 * j[:-1] + 1] = dl
    return out


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default="unknown")
    ap.add_argument("--small", action="store_true", help="N = 10^5 only (a functional check of the script)")
    ap.add_argument("--reps", type=int, default=51)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tripivot.md"))
    a = ap.parse_args()
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), device="cuda")      # noqa: E731
    lines = ["# Pivoted tridiagonal solve beside the default one", "",
             "`python scripts/tripivot_probe.py --head %s`: commit %s, %s, one process, HIP events on the context's stream, %d warm-up solves," % (a.head, a.head, torch.cuda.get_device_name(0), a.warmup),
             "median of %d (min .. max).  One diagonally dominant system (d in [2.5, 3.5], off-diagonals in [-1, 1]), (alpha, beta) = (0, 1);" % a.reps,
             "both paths return status 0.  Byte model of the pivoted solve: about 13 N doubles (104 N bytes); `model` = that at 8 TB/s.", "",
             "| N | layout | launches (pivoted) | default ms | pivoted ms | pivoted / default | model ms | pivoted GB/s by the model's bytes |", "|---|---|---|---|---|---|---|---|"]
    for N in ([10 ** 5] if a.small else [10 ** 6, 10 ** 7]):
        rng = np.random.default_rng(N)
        dl, du, d, rhs = rng.uniform(-1, 1, N - 1), rng.uniform(-1, 1, N - 1), 2.5 + rng.random(N), rng.standard_normal(N)
        for layout in ("diagonals", "csc"):
            J = fd.Tridiagonal(dev(dl), dev(d), dev(du)) if layout == "diagonals" else [dev(csc_nzval(dl, d, du))]
            b, y = dev(rhs), torch.empty(N, dtype=torch.float64, device="cuda")
            res = {}
            for piv in (False, True):
                s = fd.TridiagSolver(N, layout)
                s.set_pivoting(piv)
                res[piv] = median_ms(lambda: s.solve(J, b, y, 0.0, 1.0), a.warmup, a.reps)
                assert s.status() == 0 and bool(torch.isfinite(y).all())
            nl = len(M.piv_levels(N))
            model_ms = 104.0 * N / 8e12 * 1e3
            lines.append("| %d | %s | %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f | %.4f | %.0f |" % (
                N, layout, 2 * nl - 1, *res[False], *res[True], res[True][0] / res[False][0], model_ms, 104.0 * N / (res[True][0] * 1e-3) / 1e9))
            print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
