"""Timing of the sparse consumer (fd_csc_matvec_async / fd_csc_solve_async) in Float64: HIP events after a warm-up, the
median with min - p90, against the stream-copy ceiling measured in the same process and against torch.sparse_csr_tensor @ v on the
same matrix (its values permuted to CSR beforehand, not timed).  Writes profiles/csc_solver.md.

    python scripts/csc_solver_probe.py --head $(git rev-parse --short=12 HEAD) [--only lap5,band,tridiag] [--small]
With --trace the script starts ONE child of its own under `rocprofv3 --kernel-trace --stats` (a fresh process: one solve per pattern,
nothing else) and reads the kernel table of its trace: the per-kernel split of a solve and the COUNTED launches per enqueued
iteration.  Read-backs per solve are not in a kernel trace: that column is derived from the schedule (one record per batch of 8)."""
import argparse
import ctypes as C
import glob
import os
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import finitediff_jl_amd as fd
import csc_solve_model as M


def band_pattern(n, half, per_col, seed, chunk=50000):
    """tests/csc_solve_model.py's random band, drawn in chunks of columns (its key table is n x (2 half + 1) doubles otherwise)."""
    rng = np.random.default_rng(seed)
    off = np.arange(-half, half + 1)[None, :]
    out = []
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        keys = rng.random((c1 - c0, 2 * half + 1))
        rows = np.arange(c0, c1)[:, None] + off
        keys[(rows < 0) | (rows >= n)] = 2.0
        pick = np.sort(np.argpartition(keys, per_col, axis=1)[:, :per_col], axis=1)
        out.append(np.take_along_axis(rows, pick, axis=1).reshape(-1))
    return (np.arange(n + 1) * per_col).astype(np.int64), np.concatenate(out).astype(np.int64), n


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts = np.sort(np.array(ts))
    return float(np.median(ts)), float(ts[0]), float(ts[int(0.9 * (len(ts) - 1))])


ITER_KERNELS = ("k_cs_p", "k_cs_rows", "k_cs_long", "k_cs_s", "k_cs_update")


def traced_child(keys, small):
    """One solve per pattern in a child under rocprofv3; returns (markdown lines, launches per enqueued iteration)."""
    d = tempfile.mkdtemp(prefix="csc_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", "--only", keys]
    if small:
        cmd.append("--small")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if r.returncode != 0 or not dbs:
        return ["", "kernel trace: the child failed (exit %d)" % r.returncode, r.stderr[-400:]], None
    cur = sqlite3.connect(dbs[0]).cursor()
    cur.execute("select name, count(*), avg(duration), sum(duration) from kernels group by name order by sum(duration) desc")
    rows = [(n.replace("fdjac::", "").replace("void ", "").split("(")[0], c, a_, t) for n, c, a_, t in cur.fetchall()]
    rows = [x for x in rows if "k_cs_" in x[0]]
    tot = sum(x[3] for x in rows) or 1
    out = ["", "## Per-kernel split of the solves (one `rocprofv3 --kernel-trace --stats` child: one solve at 0.99 per pattern %s)" % keys, "",
           "| kernel | launches | avg us | total us | % |", "|---|---|---|---|---|"]
    for n, c, a_, t in rows:
        out.append("| %s | %d | %.2f | %.1f | %.1f |" % (n, c, a_ / 1e3, t / 1e3, 100.0 * t / tot))
    n_it = sum(c for n, c, _a, _t in rows if n.startswith("k_cs_p"))
    n_all = sum(c for n, c, _a, _t in rows if n.split("<")[0] in ITER_KERNELS)
    per = n_all / n_it if n_it else None
    out += ["", "Counted from that trace: %d launches of the iteration kernels over %d enqueued iterations = %s per iteration "
            "(enqueued iterations include the batch that follows convergence, whose kernels leave at once)." % (n_all, n_it, "%.2f" % per if per else "n/a")]
    for f in dbs:
        os.remove(f)
    return out, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--head", default="unknown")
    ap.add_argument("--only", default="lap5,band,tridiag")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csc_solver.md"))
    a = ap.parse_args()
    cases = {"lap5": ("5-point 4000 x 2500", lambda: M.lap5_pattern(*((400, 250) if a.small else (4000, 2500)))),
             "band": ("random band 2e6 x 6 (+-300)", lambda: band_pattern(20000 if a.small else 2 * 10 ** 6, 300, 6, 11)),
             "tridiag": ("tridiagonal 1e7", lambda: M.tridiag_pattern(10 ** 5 if a.small else 10 ** 7))}
    ctx = fd.Context.default()
    gb = C.c_double()
    fd.lib.check(ctx.L.fd_stream_copy_gbps(ctx.handle, 1 << 28, 10, C.byref(gb)))
    lines = ["# Sparse consumer: products and BiCGStab on CSC storage (Float64)", "", "head: %s" % a.head, "",
             "Stream-copy ceiling measured in this process (`fd_stream_copy_gbps`): %.0f GB/s.  Times in microseconds: median (min - p90) of %d HIP-event "
             "samples after a warm-up.  Counted bytes of a product: 16 per entry (nzval 8, slot 4, column 4) + 16 N (v, y) + 4 N (row offsets)." % (gb.value, a.reps), "",
             "## Products", "", "| pattern | N | nnz | J v us | fraction of ceiling | J^T v us | torch CSR @ v us | J v / torch |", "|---|---|---|---|---|---|---|---|"]
    solve_lines = ["", "## Solve (I - gamma J) y = b, rtol 1e-10", "",
                   "| pattern | gamma max||row||_1 | iterations | solve us | us / iteration | launches / iteration (by construction) | read-backs / solve (derived: batches of 8, one behind) | direct tridiagonal us |", "|---|---|---|---|---|---|---|---|"]
    for key in a.only.split(","):
        title, gen = cases[key]
        colptr, rowval, N = gen()
        nnz = rowval.size
        g = torch.Generator(device="cuda"); g.manual_seed(3)
        nz = torch.rand(nnz, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
        v = torch.rand(N, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
        y = torch.empty(N, dtype=torch.float64, device="cuda")
        s = fd.CscSolver((torch.as_tensor(colptr, device="cuda"), torch.as_tensor(rowval, device="cuda"), N), idx_base=0)
        row_ptr, row_col, row_slot, _diag, nlong = s.row_lists()
        csr = torch.sparse_csr_tensor(row_ptr.long(), row_col.long(), nz[row_slot.long()], size=(N, N))
        if not a.child:
            t_mv = timed(lambda: s.matvec(nz, v, y, 0.0, 1.0), a.reps)
            t_mt = timed(lambda: s.matvec(nz, v, y, 0.0, 1.0, transpose=True), a.reps)
            t_th = timed(lambda: csr @ v, a.reps)
            nbytes = 16 * nnz + 20 * N
            lines.append("| %s | %d | %d | %.1f (%.1f - %.1f) | %.2f | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.2f |" % (
                title, N, nnz, *t_mv, nbytes / (t_mv[0] * 1e-6) / 1e9 / gb.value, *t_mt, *t_th, t_mv[0] / t_th[0]))
        rowsum = torch.zeros(N, dtype=torch.float64, device="cuda").index_add_(0, torch.as_tensor(rowval, device="cuda"), nz.abs())
        b = torch.rand(N, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
        if a.child:
            gamma = 0.99 / float(rowsum.max())
            s.set_options(1e-10, 500)
            s.solve(nz, b, y, 1.0, -gamma)
            print(key, s.status())
            continue
        for target in (0.5, 0.99):
            gamma = target / float(rowsum.max())
            s.set_options(1e-10, 500)
            s.solve(nz, b, y, 1.0, -gamma)
            st = s.status()
            t_sv = timed(lambda: s.solve(nz, b, y, 1.0, -gamma), max(5, a.reps // 3), warm=2)
            batches = -(-st["iterations"] // 8) + 1
            direct = ""
            if key == "tridiag":
                ts = fd.TridiagSolver(N, layout="csc")
                t_d = timed(lambda: ts.solve([nz], b, y, alpha=1.0, beta=-gamma), a.reps)
                direct = "%.1f (%.1f - %.1f)" % t_d
            solve_lines.append("| %s | %.2f | %d (flags %d) | %.1f (%.1f - %.1f) | %.1f | %d | %d | %s |" % (
                title, target, st["iterations"], st["flags"], *t_sv, t_sv[0] / max(1, st["iterations"]), 5 + (2 if nlong else 0), batches, direct))
        del s, csr, nz, v, y
    if a.child:
        return
    trace_lines = traced_child(a.only, a.small)[0] if a.trace else []
    text = "\n".join(lines + solve_lines + trace_lines) + "\n"
    print(text)
    if not a.no_write:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
