"""The ROW-WISE hand-over decompression (FD_PLAN_HANDOVER_ROWS; k_decompress_rows, csrc/fdjac_decompress_rows.hip): k_perturb -> plain f!
(FD_F_SPARSE through the plain launcher: opaque to the plan) -> one thread per row through the plan's row lists.  The hand-over path is
forced as tests/test_gpu_exact_general.py forces it (FDJAC_SMALL=0, FDJAC_LAZY_STORE=0); no kernel switch is set, so a plan without the
flag takes the plan builder's own route.  The cases live in tests/handover_rows_cases.py (pure numpy; tests/test_handover_rows_cpu.py).

  1  every case: FD_INFO_HANDOVER_ROWS == 1, the stored values are the exact model's bits (the helper of the existing exact tests: NaN
     where the model has NaN, every other value bit for bit, the step sizes by that helper's rule), x unchanged, as many f! evaluations
     as the route without the flag
  2  every case: the same call on a plan without the flag gives the same bytes -- both outputs start from one sentinel pattern, so an
     untouched slot compares too -- and the same step sizes; the complex step (MODE 2) likewise on random_band and tiny_65, random_band
     also against the pair model of tests/exact_complex_cases.py
  3  plans that keep no row lists accept the flag, report 0 and keep their bits: a column window, a dense destination, an exact band
     without store_csc_always
  4  the flag without FD_PLAN_STORE_CSC_ROWS at the C level: FD_ERR_ARG and a message naming both flags; a dense-destination and a
     complex-x plan given all three flags at the C level create fine and report 0
  5  examples/handover_rows_client.c builds with gcc and exits 0"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exact_complex_cases as Z
import exact_general as G
import exact_model as X
import handover_rows_cases as H
from test_gpu_exact_model import _check
from finitediff_jl_amd import patterns as P
import finitediff_jl_amd as fd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("FDJAC_WINDOW", "FDJAC_WINDOW2D", "FDJAC_SORTED", "FDJAC_WIN_TILE", "FDJAC_PLAN_DEVICE", "FDJAC_ROWS_ENTS")


def _force_hand_over(monkeypatch, lazy_store="0"):
    monkeypatch.setenv("FDJAC_SMALL", "0")            # the defined two-level order of the step-size reduction at every N
    for name in SWITCHES + ("FDJAC_LAZY_STORE",):
        monkeypatch.delenv(name, raising=False)
    if lazy_store is not None:
        monkeypatch.setenv("FDJAC_LAZY_STORE", lazy_store)


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _sentinel(n, t):
    return (torch.arange(n, dtype=torch.float64, device="cuda") * 0.5 - 777.25).to(t)


def _route(plan):
    return ("rows" if plan.info(fd.lib.INFO_HANDOVER_ROWS) else "window" if plan.info(fd.lib.INFO_WINDOW) else
            "sorted" if plan.info(fd.lib.INFO_SORTED_GATHER) else "list")


def _run(case, inp, flag, fdtype=None, **plan_kw):
    """One call of the case on a fresh plan: (plan, out, x before, x after, f! evaluations)."""
    M, N, colptr, rowval, colors, dtype = (inp[k] for k in ("M", "N", "colptr", "rowval", "colors", "dtype"))
    fdtype = fdtype or case["fdtype"]
    t = torch.float64 if dtype == np.float64 else torch.float32
    kw = dict(plan_kw)
    if case["variant"] == "chunked":        # room for two colours' points and values at a time
        rnd = lambda n: (n + 31) // 32 * 32
        kw["scratch_bytes"] = 2 * (2 if fdtype == "central" else 1) * np.dtype(dtype).itemsize * (rnd(N) + rnd(M)) + 4096
    J = fd.SparseMatrixCSC(M, N, colptr, rowval)
    plan = fd.make_plan(J, J, colors, fdtype, dtype=dtype, handover_rows=flag, **kw)
    out = _sentinel(plan.out_len(0), t)
    f = fd.BuiltinF.sparse(M, N, colptr, rowval, dtype=dtype)
    x = torch.as_tensor(inp["x"], device="cuda")
    x0 = x.clone()
    f_in = None if inp.get("f_in") is None else torch.as_tensor(inp["f_in"], device="cuda")
    call = dict(f_in=f_in) if fdtype != "complex" else {}
    if fdtype != "complex":
        call.update(relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"])
    plan.jacobian(f, x, [out], **call)
    torch.cuda.synchronize()
    return plan, out, x0, x, plan.fcalls_last


@pytest.mark.parametrize("case", H.CASES, ids=[c["id"] for c in H.CASES])
def test_rows_route_against_the_model_and_the_route_without_the_flag(monkeypatch, case):
    _force_hand_over(monkeypatch)
    inp = G.inputs(case)
    C_, dtype = inp["C"], inp["dtype"]
    plan, out, x0, x1, calls = _run(case, inp, True)
    ref, out_ref, _x0, _x1, calls_ref = _run(case, inp, False)
    flags = dict(rows=plan.info(fd.lib.INFO_HANDOVER_ROWS), ref_route=_route(ref), nchunks=plan.info(fd.lib.INFO_NCHUNKS),
                 lazy_store=plan.info(fd.lib.INFO_LAZY_STORE), small=plan.info(fd.lib.INFO_SMALL_FUSED), C=plan.info(fd.lib.INFO_NCOLORS))
    print("\n%s: %s" % (case["id"], flags))
    # 1. the exact model's bits
    want = G.layout(case, inp)

    def want_checked(D):
        lay = want(D)
        assert lay[0].size == 0 or np.isfinite(lay[0]).mean() >= G.MIN_FINITE, float(np.isfinite(lay[0]).mean())
        return lay
    _check(plan, [out], want_checked, inp["x"], inp["c0"], C_, case["fdtype"], inp["rel"], inp["ab"], case["dir"], dtype, inp["f"],
           defined_order=C_ <= 8, f_in=inp["f_in"])
    assert torch.equal(_bits(x1), _bits(x0))
    assert calls == calls_ref and calls > 0, (calls, calls_ref)
    # 2. the bytes of the route without the flag, and its step sizes
    assert torch.equal(_bits(out), _bits(out_ref)), (case["id"], int((_bits(out) != _bits(out_ref)).sum()))
    assert X.same_bits(plan.epsilons().astype(dtype), ref.epsilons().astype(dtype)).all()
    # which route ran (asserted last, so that a wrong route still shows its values' verdict)
    assert flags["rows"] == 1 and flags["ref_route"] != "rows", flags
    assert ref.info(fd.lib.INFO_HANDOVER_ROWS) == 0
    assert flags["lazy_store"] == 0 and flags["small"] == 0 and flags["C"] == C_, flags
    assert (flags["nchunks"] > 1) if case["variant"] == "chunked" else (flags["nchunks"] == (1 if C_ else 0)), flags


@pytest.mark.parametrize("pat", H.COMPLEX_PATTERNS)
def test_complex_step_equals_the_list_route(monkeypatch, pat):
    _force_hand_over(monkeypatch)
    zcase = None
    if pat == "random_band":      # tests/exact_complex_cases.py has this general pattern: its inputs, and its pair model below
        zcase = next(c for c in Z.CASES if c["id"] == "handover-sparse-random_band-greedy-f64-ordinary-csc_list")
        inp = Z.inputs(zcase)
    else:
        inp = G.inputs(H._case(pat, "greedy", "forward"))
    case = dict(variant=None, fdtype="complex", dir=1.0)
    plan, out, x0, x1, calls = _run(case, inp, True, fdtype="complex")
    ref, out_ref, _x0, _x1, calls_ref = _run(case, inp, False, fdtype="complex")
    assert plan.info(fd.lib.INFO_HANDOVER_ROWS) == 1 and ref.info(fd.lib.INFO_HANDOVER_ROWS) == 0
    assert torch.equal(_bits(out), _bits(out_ref)) and torch.equal(_bits(x1), _bits(x0)) and calls == calls_ref > 0
    if zcase is not None:
        eps = X.complex_epsilons(inp["C"], inp["dtype"])
        D = X.colour_values_complex(inp["f"], inp["x"], inp["c0"], inp["C"], eps)
        lay = Z.layout(zcase, inp)(D)[0]
        m = X.same_bits(out.cpu().numpy(), lay)
        assert m.all(), (int((~m).sum()), np.nonzero(~m)[0][:6].tolist())
        assert X.same_bits(plan.epsilons().astype(inp["dtype"]), eps).all()


def test_plans_without_row_lists_accept_the_flag_and_keep_their_route(monkeypatch):
    # a column window
    _force_hand_over(monkeypatch)
    case = H._case("random_band", "greedy", "forward")
    inp = G.inputs(case)
    plan, out, _a, _b, calls = _run(case, inp, True, col_window=G.COL_WINDOW)
    ref, out_ref, _a, _b, calls_ref = _run(case, inp, False, col_window=G.COL_WINDOW)
    assert plan.info(fd.lib.INFO_HANDOVER_ROWS) == 0 and _route(plan) == _route(ref)
    assert out.numel() == int(inp["colptr"][G.COL_WINDOW[1]] - inp["colptr"][G.COL_WINDOW[0]]) and calls == calls_ref
    assert torch.equal(_bits(out), _bits(out_ref))
    # a dense destination
    M, N, colptr, rowval, colors = (inp[k] for k in ("M", "N", "colptr", "rowval", "colors"))
    outs = []
    for flag in (True, False):
        dense = torch.full((N, M), float("nan"), dtype=torch.float64, device="cuda").t()          # column-major M x N
        p = fd.make_plan(dense, fd.SparseMatrixCSC(M, N, colptr, rowval), colors, "forward", handover_rows=flag)
        assert p.info(fd.lib.INFO_HANDOVER_ROWS) == 0
        p.jacobian(fd.BuiltinF.sparse(M, N, colptr, rowval), torch.as_tensor(inp["x"], device="cuda"), [dense], relstep=inp["rel"], absstep=inp["ab"])
        outs.append(dense.contiguous())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    # an exact band without store_csc_always: its closed-form descriptors stand in for the compact copy, so there are no row lists
    # (FDJAC_LAZY_STORE unset: with it off the plan would not look for the band, and would build the lists)
    _force_hand_over(monkeypatch, lazy_store=None)
    n = 4097
    cp, rv = P.tridiag_csc(n)
    col = P.cyclic_colors(n, 3)
    x = torch.as_tensor(0.5 + 0.25 * np.sin(np.arange(1, n + 1)), device="cuda")
    got = []
    for flag in (True, False):
        J = fd.SparseMatrixCSC(n, n, cp, rv)
        p = fd.make_plan(J, J, col, "central", handover_rows=flag)
        assert p.info(fd.lib.INFO_HANDOVER_ROWS) == 0 and p.info(fd.lib.INFO_STORE_CSC) == 0
        o = _sentinel(p.out_len(0), torch.float64)
        p.jacobian(fd.BuiltinF.sparse(n, n, cp, rv), x, [o])
        got.append((o, _route(p)))
    assert got[0][1] == got[1][1] and torch.equal(_bits(got[0][0]), _bits(got[1][0]))


def test_the_flag_without_row_lists_is_an_argument_error_at_the_c_level():
    ctx = fd.Context.default()
    L = ctx.L
    M, N, colptr, rowval = G.pattern("tiny_65")
    colors = np.ascontiguousarray(G.colouring("tiny_65", "greedy"), dtype=np.int64)
    cp, rv = np.ascontiguousarray(colptr, dtype=np.int64), np.ascontiguousarray(rowval, dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def create(fn, flags):
        o = fd.lib.PlanOpts()
        o.fdtype, o.flags = fd.lib.FORWARD, flags
        h = C.c_void_p()
        rc = fn(ctx.handle, M, N, vp(cp), vp(rv), 8, 1, vp(colors), 8, C.byref(o), C.byref(h))
        return rc, h, L.fd_last_error().decode()

    def info(h):
        v = C.c_int64(-1)
        assert L.fd_plan_info(h, fd.lib.INFO_HANDOVER_ROWS, C.byref(v)) == 0
        return v.value

    R, S, HR = fd.lib.PLAN_STORE_CSC_ROWS, fd.lib.PLAN_STORE_CSC, fd.lib.PLAN_HANDOVER_ROWS
    unknown_rc, _h, unknown_msg = create(L.fd_plan_create_csc, 1 << 20)
    assert unknown_rc == 1 and "flags" in unknown_msg                              # FD_ERR_ARG: what an unknown bit gets
    for flags in (HR, HR | S):
        rc, h, msg = create(L.fd_plan_create_csc, flags)
        assert rc == unknown_rc and not h.value, (flags, rc)
        assert "flags" in msg and "FD_PLAN_HANDOVER_ROWS" in msg and "FD_PLAN_STORE_CSC_ROWS" in msg, msg
    for fn, flags, want in ((L.fd_plan_create_csc, HR | R | S, 1), (L.fd_plan_create_csc, HR | R, 0), (L.fd_plan_create_csc_dense, HR | R | S, 0),
                            (L.fd_plan_create_csc, HR | R | S | fd.lib.PLAN_COMPLEX_X, 0)):
        rc, h, msg = create(fn, flags)
        assert rc == 0 and h.value, (flags, rc, msg)
        assert info(h) == want, (flags, info(h))
        assert L.fd_plan_destroy(h) == 0


def test_the_c_client_builds_and_exits_zero(tmp_path):
    exe = str(tmp_path / "handover_rows_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "handover_rows_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-lm", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "handover_rows_client ok" in out.stdout and out.stdout.count("FD_INFO_HANDOVER_ROWS 1 / 0") == 2, out.stdout
