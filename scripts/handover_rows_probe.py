"""Kernel time and memory traffic of the ROW-WISE hand-over decompression (FD_PLAN_HANDOVER_ROWS, k_decompress_rows) against the route
the plan builder chooses without the flag, on the two general patterns the entry-ordered gathers are slowest on: the
random band (2e6 columns, 6 per column within +-300) and the 1.2e6 x 1e6 random pattern of tests/test_gpu_fullsize.py.  Float64,
forward and central, an opaque f! (FD_F_SPARSE through its plain launcher).  Writes profiles/handover_rows.md.

    python scripts/handover_rows_probe.py --head $(git rev-parse --short=12 HEAD) [--small] [--only band,rect]

The script starts three children of its own, one after the other, each a fresh process that runs the same calls:
  1  under `rocprofv3 --kernel-trace --stats`: per pattern and difference type, after WARM calls of each plan, REPS calls ALTERNATING
     between the plan with the flag and the plan without it; the decompression launches' durations are read from the trace (min, median,
     p10 - p90 spread per kernel)
  2  under `rocprofv3 --pmc FETCH_SIZE`, then under `rocprofv3 --pmc WRITE_SIZE`, and nothing else (counters only; the two do not fit the
     TCC's four slots in one pass: a child each): the same calls with fewer repetitions; the counted KiB per launch against the byte
     model below
Byte model (an estimate; Float64, 1-byte colours):
  rows route   per entry 8 (fx1 gather) + 4 (slot) + 1 (colour) + 8 (store), central 8 more (the minus point); per row 8 (row_pack) + 8 (fx, forward)
  entry route  per entry 8 (fx1 gather) + 4 (row) + 1 (colour) + 8 (store) + 8 (fx gather, or the minus point); the colour-sorted form 2 more (position)"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WARM, REPS, REPS_PMC = 3, 20, 3


def band_pattern(n, half, per_col, seed, chunk=50000):
    """A random band drawn in chunks of columns: per_col distinct rows within +-half of every column (1-based CSC)."""
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
    return n, n, (np.arange(n + 1) * per_col).astype(np.int64) + 1, np.concatenate(out).astype(np.int64) + 1


def rect_pattern(M, N, spread):
    """tests/test_gpu_fullsize.py::test_large_rectangular_random_pattern_vs_oracle's pattern (1-based CSC)."""
    rng = np.random.default_rng(1234)
    centre = (np.arange(N) * (M / N)).astype(np.int64)
    rws = centre[:, None] + rng.integers(-spread, spread + 1, size=(N, 6))
    far = rng.random(N) < 0.03
    rws[far, 0] = rng.integers(0, M, size=int(far.sum()))
    rws = np.abs(rws)
    rws = np.sort(np.where(rws > M - 1, 2 * (M - 1) - rws, rws), axis=1)
    keep = np.ones_like(rws, bool)
    keep[:, 1:] = rws[:, 1:] != rws[:, :-1]
    colptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64) + 1
    return M, N, colptr, (rws[keep] + 1).astype(np.int64)


def cases(small):
    return {"band": ("random band %s x 6 (+-300)" % ("2e4" if small else "2e6"), lambda: band_pattern(20000 if small else 2 * 10 ** 6, 300, 6, 11)),
            "rect": ("random %s" % ("1.2e4 x 1e4" if small else "1.2e6 x 1e6"),
                     lambda: rect_pattern(12000, 10000, 300) if small else rect_pattern(1_200_000, 1_000_000, 3000))}


def route(plan, fd):
    return ("k_decompress_rows" if plan.info(fd.lib.INFO_HANDOVER_ROWS) else "k_decompress_window" if plan.info(fd.lib.INFO_WINDOW) else
            "k_decompress_sorted" if plan.info(fd.lib.INFO_SORTED_GATHER) else "k_decompress_list")


def child(a):
    """The calls themselves; prints one `CASE` line per pattern and difference type (what ran, in which order)."""
    import torch
    import finitediff_jl_amd as fd
    reps = REPS if a.child == "trace" else REPS_PMC
    for key in a.only.split(","):
        title, gen = cases(a.small)[key]
        M, N, colptr, rowval = gen()
        J = fd.SparseMatrixCSC(M, N, colptr, rowval)
        colors = fd.matrix_colors(J)
        f = fd.BuiltinF.sparse(M, N, colptr, rowval)
        x = torch.as_tensor(0.5 + 0.25 * np.sin(np.arange(1, N + 1, dtype=np.float64)), device="cuda")
        for fdtype in ("forward", "central"):
            plans = {flag: fd.make_plan(J, J, colors, fdtype, handover_rows=flag) for flag in (True, False)}
            outs = {flag: torch.zeros(plans[flag].out_len(0), dtype=torch.float64, device="cuda") for flag in plans}
            assert all(p.info(fd.lib.INFO_NCHUNKS) == 1 for p in plans.values()) and route(plans[True], fd) != route(plans[False], fd)
            for flag in plans:
                for _ in range(WARM):
                    plans[flag].jacobian(f, x, [outs[flag]])
            torch.cuda.synchronize()
            for _ in range(reps):
                for flag in (True, False):
                    plans[flag].jacobian(f, x, [outs[flag]])
            torch.cuda.synchronize()
            same = torch.equal(outs[True].view(torch.int64), outs[False].view(torch.int64))
            print("CASE|%s|%s|%s|%d|%d|%d|%d|%s|%s|%d|%d|%d" % (key, title, fdtype, M, N, rowval.size, int(colors.max()), route(plans[True], fd),
                                                                route(plans[False], fd), int(same), WARM, reps), flush=True)
            del plans, outs


def run_child(mode, a):
    """The child under rocprofv3 (its csv files and its output are kept under a.raw/<mode>; a.parse_only: read what an earlier run left there)."""
    d = os.path.join(a.raw or tempfile.mkdtemp(prefix="handover_rows_"), mode)
    os.makedirs(d, exist_ok=True)
    log = os.path.join(d, "child.out")
    rc = 0
    if not a.parse_only and mode not in a.reuse.split(","):
        tool = ["--kernel-trace", "--stats"] if mode == "trace" else ["--pmc", mode]
        cmd = ["rocprofv3"] + tool + ["--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", mode,
                                      "--only", a.only] + (["--small"] if a.small else [])
        print("starting the %s child" % mode, flush=True)
        with open(log, "w") as fh:
            rc = subprocess.run(cmd, stdout=fh, stderr=subprocess.STDOUT, text=True, timeout=a.timeout).returncode
    text = open(log).read()
    meta = [ln.split("|")[1:] for ln in text.splitlines() if ln.startswith("CASE|")]
    name = "*kernel_trace.csv" if mode == "trace" else "*counter_collection.csv"
    files = glob.glob(os.path.join(d, "**", name), recursive=True)
    if rc != 0 or not files or not meta:
        raise SystemExit("the %s child failed (exit %d): %s" % (mode, rc, text[-1500:]))
    rows = []
    for fn in files:
        with open(fn, newline="") as fh:
            rows += list(csv.DictReader(fh))
    return meta, rows


def short(name):
    return name.replace("void ", "").replace("fdjac::", "").split("<")[0].split("(")[0]


def per_case(meta, rows, value):
    """The decompression dispatches in launch order, cut into the cases' runs: {(key, fdtype): {kernel: [values after the warm-up]}}."""
    order = lambda r: int(r.get("Dispatch_Id") or r.get("Start_Timestamp"))
    by_kernel = {}
    for r in sorted(rows, key=order):
        k = short(r["Kernel_Name"])
        if k.startswith("k_decompress_"):
            by_kernel.setdefault("k_decompress_window" if k.startswith("k_decompress_window") else k, []).append(value(r))
    out, at = {}, {}
    for key, _title, fdtype, _M, _N, _nnz, C, k_rows, k_ref, _same, warm, reps in meta:
        got = {}
        for k in (k_rows, k_ref):          # (one decompression launch per call: both plans hold every colour in one chunk -- the child asserts it)
            n, a0 = int(warm) + int(reps), at.get(k, 0)
            got[k] = by_kernel.get(k, [])[a0 + int(warm):a0 + n]
            at[k] = a0 + n
            if len(got[k]) != int(reps):
                raise SystemExit("%s %s: %d launches of %s in the trace, %s expected" % (key, fdtype, len(got[k]), k, reps))
        out[(key, fdtype)] = got
    return out


def stats(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return float(v[0]), float(np.median(v)), float(v[int(0.1 * (len(v) - 1))]), float(v[int(round(0.9 * (len(v) - 1)))])


def model_bytes(kernel, M, nnz, fdtype):
    if kernel == "k_decompress_rows":
        return nnz * (21 + (8 if fdtype == "central" else 0)) + M * (8 + (8 if fdtype == "forward" else 0))
    return nnz * (29 + (2 if kernel == "k_decompress_sorted" else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--head", default="unknown")
    ap.add_argument("--only", default="band,rect")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--raw", default="", help="keep the children's csv files and output under this directory")
    ap.add_argument("--reuse", default="", help="children (trace, FETCH_SIZE, WRITE_SIZE) whose files under --raw are read instead of run again")
    ap.add_argument("--parse-only", action="store_true", help="write the profile from what an earlier run left under --raw")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "handover_rows.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    meta, trace = run_child("trace", a)
    times = per_case(meta, trace, lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    counted = {}
    for name in ("FETCH_SIZE", "WRITE_SIZE"):
        meta_p, pmc = run_child(name, a)
        counted[name] = per_case(meta_p, [r for r in pmc if r["Counter_Name"] == name], lambda r: float(r["Counter_Value"]))
    fetch, write = counted["FETCH_SIZE"], counted["WRITE_SIZE"]
    L = ["# Hand-over decompression row by row (FD_PLAN_HANDOVER_ROWS) against the plan builder's route", "", "head: %s" % a.head, "",
         "Float64, an opaque f! (FD_F_SPARSE, plain launcher).  Kernel times in microseconds from ONE `rocprofv3 --kernel-trace --stats` child: per pattern "
         "and difference type %d warm-up calls of each plan, then %d calls ALTERNATING between the plan with the flag and the plan without it "
         "(the parent's automatic route, named in the table), same process, same box; min / median / p10 - p90 of the decompression launch alone."
         % (WARM, REPS), "",
         "| pattern | fdtype | M | nnz | colours | route without the flag: min / median (p10 - p90) | k_decompress_rows: min / median (p10 - p90) | rows / route (medians) | same bytes |",
         "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for key, title, fdtype, M, N, nnz, C, k_rows, k_ref, same, _w, _r in meta:
        t = times[(key, fdtype)]
        a_, b_ = stats(t[k_ref]), stats(t[k_rows])
        ratio = b_[1] / a_[1]
        spread = max((a_[3] - a_[2]) / a_[1], (b_[3] - b_[2]) / b_[1])
        verdicts.append((title, fdtype, ratio, spread))
        L.append("| %s | %s | %s | %s | %s | %s: %.1f / %.1f (%.1f - %.1f) | %.1f / %.1f (%.1f - %.1f) | %.3f | %s |" % (
            title, fdtype, M, nnz, C, k_ref, a_[0], a_[1], a_[2], a_[3], b_[0], b_[1], b_[2], b_[3], ratio, "yes" if same == "1" else "NO"))
    L += ["", "Verdict per line (a difference counts only beyond the larger p10 - p90 spread of the two, relative to the median):", ""]
    for title, fdtype, ratio, spread in verdicts:
        what = "faster" if ratio < 1 - spread else "slower" if ratio > 1 + spread else "no faster (within the spread)"
        L.append("- %s, %s: rows / route = %.3f, spread %.3f: the row route is measured **%s**" % (title, fdtype, ratio, spread, what))
    L += ["", "## Counted traffic", "",
          "SEPARATE counters-only children (`rocprofv3 --pmc FETCH_SIZE`, then `rocprofv3 --pmc WRITE_SIZE`, no tracing), %d alternating calls after the warm-up; medians per launch, "
          "in MB (counter x 1024 B), against the byte model in the script's docstring (an estimate: the gathers are counted at 8 B, not at sector "
          "granularity)." % REPS_PMC, "",
          "| pattern | fdtype | kernel | FETCH MB | WRITE MB | model MB | counted / model |", "|---|---|---|---|---|---|---|"]
    for key, title, fdtype, M, N, nnz, C, k_rows, k_ref, same, _w, _r in meta_p:
        for k in (k_ref, k_rows):
            fm = float(np.median(fetch[(key, fdtype)][k])) * 1024 / 1e6
            wm = float(np.median(write[(key, fdtype)][k])) * 1024 / 1e6
            mb = model_bytes(k, int(M), int(nnz), fdtype) / 1e6
            L.append("| %s | %s | %s | %.1f | %.1f | %.1f | %.2f |" % (title, fdtype, k, fm, wm, mb, (fm + wm) / mb))
    text = "\n".join(L) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
