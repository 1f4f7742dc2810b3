#!/usr/bin/env python3
"""Device column colouring (fd_color_columns_device) against the route it replaces for a pattern that lives on the device: copy
colptr / rowval to the host, fd_color_columns_greedy, copy the colours back.  Both in this process, on the same arrays.  Host wall
clock around each call with the device idle before it (the call synchronises itself; HIP events cannot bracket it), median of
--reps calls after --warmup.  Rounds and launches come from the library's own count (FDJAC_COLOR_STATS, one extra untimed call).
Prints a markdown table.  Every pattern runs in a child process under its own time limit; the first failure ends the probe.
    python scripts/color_probe.py [--reps 20] [--warmup 3] [--only tridiag|lap5|band]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/color_probe.py --only band --reps 3 --child band"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FDJAC_TEST_SWITCHES", "1")   # (the library honours its variant switches only on request)

LIMIT_S = {"tridiag": 400, "lap5": 500, "band": 400}


def pattern(name):
    from finitediff_jl_amd import patterns as P
    if name == "tridiag":
        N = 10_000_000
        return "tridiagonal N = 10^7", N, N, P.tridiag_csc(N)
    if name == "lap5":
        N = 4000 * 2500
        return "5-point 4000 x 2500", N, N, P.lap5_csc(4000, 2500)
    N = 2_000_000                                   # the random band of scripts/terms_probe.py
    rng = np.random.default_rng(1)
    offs = np.sort(rng.integers(-300, 301, size=(N, 6)), axis=1)
    rows = np.arange(N)[:, None] + offs
    keep = (rows >= 0) & (rows < N)
    keep[:, 1:] &= rows[:, 1:] != rows[:, :-1]
    colptr = np.empty(N + 1, np.int64)
    colptr[0] = 1
    np.cumsum(keep.sum(axis=1), out=colptr[1:])
    colptr[1:] += 1
    return "random band 2*10^6 x 6 (+-300)", N, N, (colptr, (rows[keep] + 1).astype(np.int64))


def stats_line(call):
    """Run `call` once with FDJAC_COLOR_STATS=1 and return the line the library wrote to stderr."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        os.environ["FDJAC_COLOR_STATS"] = "1"
        try:
            call()
        finally:
            os.environ.pop("FDJAC_COLOR_STATS")
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode("utf-8", "replace")


def child(name, reps, warmup):
    import ctypes as C
    import torch
    import finitediff_jl_amd as fd
    title, M, N, (colptr, rowval) = pattern(name)
    cp, rv = torch.as_tensor(colptr, device="cuda"), torch.as_tensor(rowval, device="cuda")
    L = fd.lib.load()

    def device():
        return fd.matrix_colors_device(M, N, cp, rv)

    def host_route():      # what a caller with a device-resident pattern does without fd_color_columns_device
        hc, hr = cp.cpu().numpy(), rv.cpu().numpy()
        out, nc = np.empty(N, np.int64), C.c_int64()
        fd.lib.check(L.fd_color_columns_greedy(M, N, hc.ctypes.data_as(C.c_void_p), hr.ctypes.data_as(C.c_void_p), 8, 1,
                                               out.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(nc)))
        return torch.as_tensor(out, device="cuda"), int(nc.value)

    def median_ms(fn, reps):
        ts = []
        for k in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            if k >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), r

    d_med, d_min, d_max, (dcol, dnc) = median_ms(device, reps)
    bad = fd.check_colors_device(M, N, cp, rv, dcol)
    h_med, h_min, h_max, (hcol, hnc) = median_ms(host_route, max(3, reps // 4))
    line = stats_line(device)
    m = re.search(r"rounds=(\d+) tail_levels=(\d+) round_launches=(\d+) read_backs=(\d+)", line)
    rounds, tail, launches, reads = (int(g) for g in m.groups()) if m else (-1, -1, -1, -1)
    print("| %s | %d | %d | %.2f (%.2f .. %.2f) | %.1f (%.1f .. %.1f) | %.1fx | %d | %d | %d | %d | %d | %d | %d |"
          % (title, N, rowval.size, d_med, d_min, d_max, h_med, h_min, h_max, h_med / d_med, dnc, hnc, rounds, tail, launches, reads, bad), flush=True)
    return 0 if bad == 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup)
    print("| pattern | N | nnz | device ms: median (min .. max) | host route ms: median (min .. max) | host / device | colours device | colours host greedy "
          "| rounds | tail levels | launches (rounds + tail + output) | read-backs | rows with a repeated colour |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for name in ("tridiag", "lap5", "band"):
        if a.only and a.only != name:
            continue
        try:      # a fresh process per pattern, under its own time limit; nothing more is started after a failure
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                                timeout=LIMIT_S[name]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("color_probe: %s ended with status %d; stopping" % (name, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
