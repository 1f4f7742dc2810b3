"""Times the objective Hessian / gradient kernels (fd_hessian_async / fd_gradient_async) on two partially separable objectives:
  chain   N = 10^6, phi_r reads x[r-1], x[r], x[r+1]; H into BandedMatrix data (l = u = 2)
  grid5   2000 x 2000, phi_r reads the 5-point neighbourhood of node r; H into the nzval of P (CSC)
with HIP events around each enqueued call (warm-up first; median and spread of the samples), and prints one JSON object with the
per-call microseconds, the counted-bytes model of every pass and the fraction of the measured stream-copy ceiling it reaches.

    python scripts/hessian_probe.py [--iters 50] [--warmup 10] [--only chain|grid5] [--out FILE]

For the per-kernel split run it once under `rocprofv3 --kernel-trace --stats -- python scripts/hessian_probe.py --iters 20`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import finitediff_jl_amd as fd  # noqa: E402
from finitediff_jl_amd import lib as L_  # noqa: E402
from finitediff_jl_amd import patterns as P  # noqa: E402

import hess_model as hm  # noqa: E402


def _time(torch, call, iters, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in evs])
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "p90_us": float(np.percentile(us, 90))}


def run(name, torch, iters, warmup, ceiling_gbps):
    if name == "chain":
        n = 1_000_000
        cp, rv = hm.chain_support(n)
        M, N, src, typ, params, dest = n, n, hm.CHAIN_SRC, "Chain", np.int64(n).tobytes(), "banded"
    else:
        nx = ny = 2000
        cp, rv = P.lap5_csc(nx, ny)
        cp, rv = cp - 1, rv - 1
        M = N = nx * ny
        src, typ, params, dest = hm.GRID5_SRC, "Grid5", np.array([nx, ny], np.int64).tobytes(), "csc"
    S = fd.SparseMatrixCSC(M, N, cp + 1, rv + 1)
    f = fd.ObjectiveF(src, typ, M, N, params=params)
    x = torch.as_tensor(np.random.default_rng(0).uniform(-1, 1, N), device="cuda:0")
    hc = fd.HessianCache(x, S, dest=dest)
    nnz, nent, lst, out_len = (hc.info(k) for k in (L_.HESS_INFO_NNZ, L_.HESS_INFO_UPPER, L_.HESS_INFO_LIST_LEN, L_.HESS_INFO_OUT_LEN))
    H = torch.zeros(out_len, dtype=torch.float64, device="cuda:0")
    if dest == "banded":
        H = fd.BandedMatrix(H.reshape(N, 2 * hc.band + 1).t(), N, hc.band, hc.band)
    g = torch.zeros(N, dtype=torch.float64, device="cuda:0")
    gf, gc = fd.GradientCache(x, "forward", S), fd.GradientCache(x, "central", S)
    res = {"M": M, "N": N, "dest": dest, "nnz_P": nnz, "upper_entries": nent, "list_len": lst, "nnz_S": int(rv.size)}
    res["hessian"] = _time(torch, lambda: fd.finite_difference_hessian_b(H, f, x, hc), iters, warmup)
    res["gradient_forward"] = _time(torch, lambda: fd.finite_difference_gradient_b(g, f, x, gf), iters, warmup)
    res["gradient_central"] = _time(torch, lambda: fd.finite_difference_gradient_b(g, f, x, gc), iters, warmup)
    # counted bytes: every array the passes must touch once (x and fx gathers counted once per element: the ideal reuse)
    rows_b = 8 * N + 8 * M                                           # x read, fx written
    entry_b = 16 * nent + 8 + 4 * lst + 8 * N + 8 * M + 8 * out_len  # i, j, lo (+1) per entry; rows; x; fx; H written
    if dest == "csc":
        entry_b += 16 * nent                                         # the two destination slots of every entry
    zero_b = 8 * (2 * hc.band + 1) * 2 * hc.band if dest == "banded" else 0      # the corner columns' zero fill
    grad_b = 8 * (N + 1) + 4 * int(rv.size) + 8 * N + 8 * N          # S colptr, rowval; x; g written
    res["bytes"] = {"rows_pass": rows_b, "entry_pass": entry_b, "zero_fill": zero_b, "hessian": rows_b + entry_b + zero_b,
                    "gradient_forward": rows_b + grad_b + 8 * M, "gradient_central": grad_b,
                    "floor_per_column_chain": 64 if name == "chain" else None}
    for k in ("hessian", "gradient_forward", "gradient_central"):
        gbps = res["bytes"][k] / (res[k]["median_us"] * 1e-6) / 1e9
        res[k]["counted_GBps"] = gbps
        res[k]["fraction_of_copy_ceiling"] = gbps / ceiling_gbps
    res["hessian"]["per_column_bytes"] = res["bytes"]["hessian"] / N
    res["objective_launches"] = f.launches
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=["chain", "grid5"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    ctx = fd.Context.default()
    ceiling = ctx.stream_copy_gbps(1 << 30, 10)
    out = {"copy_ceiling_GBps": ceiling}
    for name in ("chain", "grid5"):
        if a.only in (None, name):
            out[name] = run(name, torch, a.iters, a.warmup, ceiling)
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s)


if __name__ == "__main__":
    main()
