"""Timing of the block-Jacobi preconditioner of the sparse consumer (fd_csc_solver_set_preconditioner) in Float64 beside the
diagonal one, in the same process: HIP events, 10 warm-up and 50 timed solves, the median with min - p90.  Cases: the reaction-diffusion
family of tests/csc_block_model.py with m = 8 species on 1000 x 1000 cells (built on the device), and the block-tridiagonal pattern
with 32 x 32 blocks.  Writes profiles/csc_precond.md.

The fixed part of a solve.  With b = 0 and max_iterations = 1 a solve is its fixed part: the start kernel (which finds ||b|| = 0 and
sets `done`), with the blocks k_cs_binv (it does not look at `done`), ONE iteration's kernels, which leave at once, one record and the
final kernel.  It is timed for either preconditioner.  "us / iteration" is (solve - fixed part) / iterations.  The C ABI has no entry
that enqueues k_cs_binv alone, so between HIP events the gather-and-invert launch is the DIFFERENCE of the two fixed parts: k_cs_binv
plus two more kernels that leave at once (the applies), minus the diagonal that only the Jacobi start kernel forms.  The trace below has
the kernel's own duration.

    python scripts/csc_precond_probe.py --head $(git rev-parse --short=12 HEAD) [--small] [--trace]
With --trace the script starts one child of its own per preconditioner under `rocprofv3 --kernel-trace --stats` (a fresh process: one
solve per case, nothing else; no counters in those runs) and reads the kernel table of each trace: the per-kernel split, k_cs_binv's
own time and the COUNTED launches per enqueued iteration."""
import argparse
import ctypes as C
import glob
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import finitediff_jl_amd as fd
import csc_block_model as BM

GAMMA = 0.1
T0 = time.time()


def note(*what):
    """Progress on stderr: a run of several minutes is not silent."""
    print("[%6.1f s]" % (time.time() - T0), *what, file=sys.stderr, flush=True)


def family_on_device(nx, ny, m, k, cond, skew, seed):
    """tests/csc_block_model.py's reaction_diffusion with torch on the device (its QR loop over 10^6 cells is a host minute otherwise):
    the same pattern and the same law of the values, not the same random numbers.  0-based Int32 colptr / rowval, Float64 nzval."""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    dev, ncell, N = "cuda", nx * ny, nx * ny * m
    c = torch.linspace(0.5, 1.5, m, dtype=torch.float64, device=dev)
    lam = torch.logspace(-np.log10(cond), 0.0, m, dtype=torch.float64, device=dev)
    G = torch.randn(ncell, m, m, generator=g, dtype=torch.float64, device=dev)
    Q = torch.empty_like(G)                     # Gram-Schmidt on the columns of G: the Q of its QR (torch.linalg.qr walks the batch on the host)
    for j in range(m):
        v = G[:, :, j].clone()
        for i in range(j):
            v -= (Q[:, :, i] * v).sum(dim=1, keepdim=True) * Q[:, :, i]
        Q[:, :, j] = v / v.norm(dim=1, keepdim=True)
    del G
    H = torch.randn(ncell, m, m, generator=g, dtype=torch.float64, device=dev)
    R = -k * ((Q * lam) @ Q.transpose(1, 2) + skew * 0.5 * (H - H.transpose(1, 2)))
    R.diagonal(dim1=1, dim2=2).add_(-4.0 * c)
    cell = torch.arange(ncell, device=dev)
    ci, cj = cell % nx, cell // nx
    s = torch.arange(m, device=dev)
    rows = torch.full((ncell, m, m + 4), -1, dtype=torch.int64, device=dev)
    vals = torch.zeros((ncell, m, m + 4), dtype=torch.float64, device=dev)
    for slot, nb, ok in ((0, cell - nx, cj > 0), (1, cell - 1, ci > 0), (m + 2, cell + 1, ci < nx - 1), (m + 3, cell + nx, cj < ny - 1)):
        rows[:, :, slot] = torch.where(ok[:, None], nb[:, None] * m + s[None, :], torch.full_like(rows[:, :, slot], -1))
        vals[:, :, slot] = c[None, :]
    rows[:, :, 2:m + 2] = (cell[:, None] * m + s[None, :])[:, None, :]
    vals[:, :, 2:m + 2] = R.transpose(1, 2)
    keep = rows >= 0
    colptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), keep.reshape(N, -1).sum(dim=1).cumsum(0)])
    return colptr.to(torch.int32), rows[keep].to(torch.int32), vals[keep].contiguous(), N


def block_tridiag_on_device(nblk, bs, seed):
    colptr, rowval, N = BM.block_tridiag_pattern(nblk, bs)
    cols = np.repeat(np.arange(N), np.diff(colptr))
    nz = np.random.default_rng(seed).uniform(-1, 1, rowval.size) * np.where(rowval // bs == cols // bs, 1.0, 0.05)
    return (torch.as_tensor(colptr.astype(np.int32), device="cuda"), torch.as_tensor(rowval.astype(np.int32), device="cuda"),
            torch.as_tensor(nz, device="cuda"), N)


def timed(fn, reps=50, warm=10):
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


ITER_KERNELS = ("k_cs_p", "k_cs_bapply", "k_cs_rows", "k_cs_long", "k_cs_s", "k_cs_update")


def traced_child(kind, small):
    """One solve per case with the preconditioner `kind` in a child under rocprofv3 -> markdown lines."""
    d = tempfile.mkdtemp(prefix="csc_precond_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", kind]
    if small:
        cmd.append("--small")
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=500)          # (its progress goes to this process's stderr)
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if r.returncode != 0 or not dbs:
        return ["", "kernel trace (%s): the child failed (exit %d)" % (kind, r.returncode), r.stdout[-400:]]
    cur = sqlite3.connect(dbs[0]).cursor()
    cur.execute("select name, count(*), avg(duration), sum(duration) from kernels group by name order by sum(duration) desc")
    rows = [(n.replace("fdjac::", "").replace("void ", "").split("(")[0], c, a_, t) for n, c, a_, t in cur.fetchall()]
    rows = [x for x in rows if "k_cs_" in x[0]]
    tot = sum(x[3] for x in rows) or 1
    out = ["", "## Per-kernel split, %s (a `rocprofv3 --kernel-trace --stats` child: one solve per case)" % kind, "",
           "| kernel | launches | avg us | total us | % |", "|---|---|---|---|---|"]
    for n, c, a_, t in rows:
        out.append("| %s | %d | %.2f | %.1f | %.1f |" % (n, c, a_ / 1e3, t / 1e3, 100.0 * t / tot))
    n_it = sum(c for n, c, _a, _t in rows if n.split("<")[0] == "k_cs_p")
    n_all = sum(c for n, c, _a, _t in rows if n.split("<")[0] in ITER_KERNELS)
    out += ["", "Counted from that trace: %d launches of the iteration kernels over %d enqueued iterations = %s per iteration "
            "(both cases together; the block-tridiagonal case has long rows: + 2; enqueued iterations include the batch that follows "
            "convergence, whose kernels leave at once)." % (n_all, n_it, "%.2f" % (n_all / n_it) if n_it else "n/a")]
    for f in dbs:
        os.remove(f)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("jacobi", "block_jacobi"), default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--head", default="unknown")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csc_precond.md"))
    a = ap.parse_args()
    cases = [("reaction-diffusion m = 8, %s cells" % ("100 x 100" if a.small else "1000 x 1000"), 8,
              lambda: family_on_device(*((100, 100) if a.small else (1000, 1000)), 8, 1e3, 1e3, 0.0, 5)),
             ("block-tridiagonal 32 x 32, %d blocks" % (1000 if a.small else 30000), 32, lambda: block_tridiag_on_device(1000 if a.small else 30000, 32, 12))]
    ctx = fd.Context.default()
    gb = C.c_double()
    fd.lib.check(ctx.L.fd_stream_copy_gbps(ctx.handle, 1 << 28, 10, C.byref(gb)))
    lines = ["# Sparse consumer: block-Jacobi against Jacobi preconditioning (Float64)", "", "head: %s" % a.head, "",
             "Stream-copy ceiling measured in this process (`fd_stream_copy_gbps`): %.0f GB/s.  Times in microseconds: median (min - p90) of 50 HIP-event "
             "samples after 10 warm-up solves; (I - 0.1 J) y = b, rtol 1e-10.  Fixed part: the same solve with b = 0 and max_iterations = 1 (start kernel, "
             "with the blocks k_cs_binv, one iteration's kernels that leave at once, one record, final kernel).  us / iteration = (solve - fixed part) / "
             "iterations: it holds the record reads of the later batches and the kernels of the batch behind convergence.  The apply moves "
             "(bs + 2) 8 N bytes per call, two calls per iteration." % gb.value, "",
             "| case | N | preconditioner | iterations (flags) | solve us | fixed part us | us / iteration | apply bytes / iteration | the same at the ceiling us |",
             "|---|---|---|---|---|---|---|---|---|"]
    inv_lines = ["", "## The gather-and-invert launch between HIP events", "",
                 "Fixed part with the blocks minus fixed part with the diagonal (medians): k_cs_binv + two applies that leave at once - the diagonal of the "
                 "Jacobi start kernel.", "", "| case | blocks | block size | fixed part, blocks us | fixed part, diagonal us | difference us |", "|---|---|---|---|---|---|"]
    for title, bs, gen in cases:
        note(title, "generating")
        cp, rv, nz, N = gen()
        torch.cuda.synchronize()
        note(title, "N = %d nnz = %d: creating the solver" % (N, rv.numel()))
        g = torch.Generator(device="cuda"); g.manual_seed(3)
        b = torch.randn(N, generator=g, device="cuda", dtype=torch.float64)
        zero = torch.zeros(N, dtype=torch.float64, device="cuda")
        y = torch.empty(N, dtype=torch.float64, device="cuda")
        s = fd.CscSolver((cp, rv, N), idx_base=0)
        fixed = {}
        for kind in ("jacobi", "block_jacobi") if a.child is None else (a.child,):
            s.set_preconditioner(kind, bs)
            s.set_options(1e-10, 500)
            s.solve(nz, b, y, 1.0, -GAMMA)
            st = s.status()
            note(title, kind, st)
            if a.child:
                print(title, kind, st)
                continue
            t = timed(lambda: s.solve(nz, b, y, 1.0, -GAMMA))
            s.set_options(1e-10, 1)
            t0 = fixed[kind] = timed(lambda: s.solve(nz, zero, y, 1.0, -GAMMA))
            st0 = s.status()
            assert st0["flags"] == 0 and st0["iterations"] == 0, st0
            nbytes = 2 * (bs + 2) * 8 * N if kind == "block_jacobi" else 0
            lines.append("| %s | %d | %s | %d (%d) | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.1f | %d | %.1f |" % (
                title, N, kind, st["iterations"], st["flags"], *t, *t0, (t[0] - t0[0]) / max(1, st["iterations"]), nbytes, nbytes / gb.value / 1e3))
        if not a.child:
            inv_lines.append("| %s | %d | %d | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.1f |" % (
                title, (N + bs - 1) // bs, bs, *fixed["block_jacobi"], *fixed["jacobi"], fixed["block_jacobi"][0] - fixed["jacobi"][0]))
        del s, cp, rv, nz, b, y, zero
    if a.child:
        return
    trace = []
    for kind in ("jacobi", "block_jacobi") if a.trace else ():
        note("traced child:", kind)
        trace += traced_child(kind, a.small)
    text = "\n".join(lines + inv_lines + trace) + "\n"
    print(text)
    if not a.no_write:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
