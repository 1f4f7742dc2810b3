"""The COMPLEX STEP on every Jacobian route of the rational built-in families against the pair model of tests/exact_model.py, bit for
bit: the hand-over path (k_perturb MODE 2 -> complex f! -> the imag-only decompression) into CSC (list / window kernels), BandedMatrix,
Tridiagonal and dense J, the tridiagonal and 5-point lazy-point launchers (imaginary parts only / (re, im) pairs), the column stores
(k_csc_store_cols_cplx for the sparse residual and the 7-point family, fd_csc_store_cols_cplx for a runtime-compiled row functor and a
runtime-compiled terms functor) and the dense uncoloured arm.  The cases live in tests/exact_complex_cases.py (pure numpy;
tests/test_exact_complex_cpu.py evaluates every one with the model alone).  Every case asserts that its route ran and that the plan's
step sizes are eps(T) in every colour; test_every_route_was_asserted reports the counts.

The promise: an unperturbed coordinate is the pair (x_j, +0), a perturbed one (x_j, eps); the residual in the pair arithmetic of `cd` /
fd_cplx<T> (complex * complex as (ar br - ai bi, ar bi + ai br); scalar * complex, complex +- scalar and complex / scalar component-wise;
-ffp-contract=off); the stored value is the imaginary part's IEEE quotient by eps.  Under an invalid colouring the COLOUR's point is
promised (the column kernels switch from the column's point to it).

The block-coupled residual (sin, cos, sinh) cannot be matched bit for bit: k_f_blockcoupled_store and its hand-over path are held to
the per-entry bound of tests/blockcoupled_bound.py against an mpmath value (the derivation stands there)."""
import struct

import numpy as np
import pytest

import exact_complex_cases as Z
import exact_model as X
import hess_model
from test_gpu_exact_model import _tridiag_outs, _tridiag_storage
from test_gpu_exact_store import SPARSE_ROWS
from test_gpu_jit import SPARSE_TERMS
import finitediff_jl_amd as fd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ASSERTED = {"hand-over, list decompression": 0, "hand-over, window decompression": 0, "hand-over, banded": 0, "hand-over, tridiagonal": 0,
            "hand-over, dense J": 0, "lazy points, imag only": 0, "lazy points, pairs": 0, "column store, sparse": 0, "column store, lap7": 0,
            "JIT row functor": 0, "JIT terms functor": 0, "dense uncoloured arm": 0}
RAN = []
COMPILED = {}      # the first functor of each compiled text and element type, kept: the library drops a module with its last functor
SWITCHES = ("FDJAC_WINDOW", "FDJAC_WINDOW2D", "FDJAC_SORTED", "FDJAC_WIN_TILE", "FDJAC_PLAN_DEVICE", "FDJAC_LAZY_STORE", "FDJAC_ROWS_ENTS")


def _functor(case, inp, plan, keep):
    route, dtype = case["route"], inp["dtype"]
    M, N, colptr, rowval = (inp[k] for k in ("M", "N", "colptr", "rowval"))
    if route == "jit":
        rp, rc = hess_model.rows_of(M, N, colptr - 1, rowval - 1)
        rp_d, rc_d = torch.as_tensor(rp, device="cuda"), torch.as_tensor(rc, device="cuda")
        keep += [rp_d, rc_d]
        f = fd.JitF(SPARSE_ROWS, "SparseRows", M, N, params=struct.pack("PP", rp_d.data_ptr(), rc_d.data_ptr()), dtype=dtype)
        COMPILED.setdefault(("rows", np.dtype(dtype).name), (f, rp_d, rc_d))
        return f
    if route == "terms":
        f = fd.JitTerms(SPARSE_TERMS, "SparseTerms", plan)
        COMPILED.setdefault(("terms", np.dtype(dtype).name), f)
        return f
    if case["fixture"] == "sparse":
        return fd.BuiltinF.sparse(M, N, colptr, rowval, dtype=dtype)
    return fd.BuiltinF(case["fixture"], *Z.fixture_params(case), dtype=dtype)


def _launches(f):
    return f.launches if isinstance(f, fd.JitF) else f.counts()[0]


@pytest.mark.parametrize("case", Z.CASES, ids=[c["id"] for c in Z.CASES])
def test_complex_step_route_against_the_model(monkeypatch, case):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("FDJAC_SMALL", "0")
    route, dest = case["route"], case["dest"]
    if route in ("handover", "dense"):
        monkeypatch.setenv("FDJAC_LAZY_STORE", "0")
        monkeypatch.setenv("FDJAC_WINDOW", "1" if dest == "csc_window" else "0")
        monkeypatch.setenv("FDJAC_WINDOW2D", "0")
        monkeypatch.setenv("FDJAC_SORTED", "0")
    inp = Z.inputs(case)
    M, N, colptr, rowval, colors, C, dtype = (inp[k] for k in ("M", "N", "colptr", "rowval", "colors", "C", "dtype"))
    t = torch.float64 if dtype == np.float64 else torch.float32
    it = torch.int64 if dtype == np.float64 else torch.int32
    eps = X.complex_epsilons(C, dtype)
    D = X.colour_values_complex(inp["f"], inp["x"], inp["c0"], C, eps)
    x = torch.as_tensor(inp["x"], device="cuda")
    x_before = x.clone()
    keep = []
    label = None
    for part in Z.parts(case, C):
        fill = (lambda n: torch.zeros((n,), dtype=t, device="cuda")) if part is not None else (lambda n: torch.full((n,), float("nan"), dtype=t, device="cuda"))
        kw = dict(dtype=dtype)
        if part is not None:
            kw["color_range"] = part
        if dest == "colwindow":
            kw["col_window"] = Z.COL_WINDOW
        if route in ("cols", "jit"):
            kw["store_csc"] = True
        if route == "terms":
            kw["store_rows"] = True
        if dest in ("banded", "tridiagonal"):
            J = _tridiag_storage(dest, N, dtype)
            plan = fd.make_plan(J, J, colors, "complex", **kw)
            outs = _tridiag_outs(J)
        elif dest == "dense":
            dense = torch.full((N, M), float("nan"), dtype=t, device="cuda").t()          # column-major M x N
            sp = None if route == "dense" else fd.SparseMatrixCSC(M, N, colptr, rowval)
            plan = fd.make_plan(dense, sp, colors, "complex", **kw)
            outs = [dense]
        else:
            J = fd.SparseMatrixCSC(M, N, colptr, rowval)
            plan = fd.make_plan(J, J, colors, "complex", **kw)
            outs = [fill(plan.out_len(0))]
        f = _functor(case, inp, plan, keep)
        if route == "lazy":
            assert getattr(f, "lazy_fn", None) is not None
            plan.set_lazy(f, imag_only=case["imag_only"], store=False)
        elif route in ("cols", "jit", "terms"):
            plan.set_lazy(f)
        want_store = 1 if route in ("cols", "jit", "terms") else 0
        assert plan.info(fd.lib.INFO_LAZY_STORE) == want_store, (case["id"], plan.info(fd.lib.INFO_LAZY_STORE))
        window = plan.info(fd.lib.INFO_WINDOW)
        if route in ("handover", "dense"):      # the decompression kernel the case names
            assert window == (1 if dest == "csc_window" else 0), (case["id"], window)
        if route == "dense":                    # the dense uncoloured arm: no pattern, every column a colour of its own, all M N slots stored
            assert plan.out_len(0) == M * N and plan.info(fd.lib.INFO_SORTED_GATHER) == 0, case["id"]
        before = _launches(f)
        plan.enable_timing(2)
        plan.jacobian(f, x, outs)
        torch.cuda.synchronize()
        perturbs = plan.timings()["perturb"]["launches"]
        plan.enable_timing(0)
        after = _launches(f)
        # the step sizes: eps(T) in every colour
        got_eps = plan.epsilons().astype(dtype)
        assert plan.info(fd.lib.INFO_NCOLORS) == C and X.same_bits(got_eps, eps).all(), (case["id"], got_eps[:4])
        # the stored values
        for o, lay in zip(outs, Z.layout(case, inp, part)(D)):
            g = o.cpu().numpy() if dest != "dense" else np.asfortranarray(o.cpu().numpy())
            m = X.same_bits(g, lay)
            assert m.all(), (case["id"], int((~m).sum()), np.argwhere(~m)[:6].tolist(), g[~m][:6].tolist(), lay[~m][:6].tolist())
        assert torch.equal(x.view(it), x_before.view(it))
        # which route ran
        if route == "dense":
            assert plan.fcalls_last == N == C, (case["id"], plan.fcalls_last)                      # one evaluation per column
        if route in ("handover", "dense"):
            assert perturbs >= 1 and after > before, (case["id"], perturbs, before, after)        # the points were materialised, f! was launched on them
            label = ("dense uncoloured arm" if route == "dense" else "hand-over, dense J" if dest == "dense" else "hand-over, banded" if dest == "banded" else
                     "hand-over, tridiagonal" if dest == "tridiagonal" else "hand-over, window decompression" if window == 1 else "hand-over, list decompression")
        elif route == "lazy":
            assert perturbs == 0 and after > before, (case["id"], perturbs, before, after)          # no materialised point: the launcher formed them
            label = "lazy points, imag only" if case["imag_only"] else "lazy points, pairs"
        else:
            assert perturbs == 0, (case["id"], perturbs)
            if route == "cols":
                assert plan.info(fd.lib.INFO_STORE_LAUNCH) == fd.lib.STORE_LAUNCH_FAMILY, (case["id"], plan.info(fd.lib.INFO_STORE_LAUNCH))
                label = "column store, lap7" if case["fixture"] == "lap7" else "column store, sparse"
            else:
                assert after - before == 1, (case["id"], before, after)                         # ONE launch of the functor's column store
                label = "JIT row functor" if route == "jit" else "JIT terms functor"
    ASSERTED[label] += 1
    RAN.append((case["id"], route, case["dtype"], case["family"]))


def test_every_route_was_asserted():
    # the module's report: per route, the cases whose assertion that the route ran has passed (a run of a selection reports only)
    print("\ncomplex-step routes asserted:", ASSERTED)
    assert sum(ASSERTED.values()) == len(RAN)
    if len(RAN) == len(Z.CASES):
        assert all(n > 0 for n in ASSERTED.values()), ASSERTED
        ran = {(route, dt, fam) for _id, route, dt, fam in RAN}
        for fam in Z.FAMILIES64:
            for route in ("handover", "lazy", "cols", "jit", "terms"):
                assert (route, "f64", fam) in ran, (route, fam)
        for fam in Z.FAMILIES32:
            for route in ("handover", "lazy", "cols", "jit", "terms"):
                assert (route, "f32", fam) in ran, (route, fam)


# ---- the block-coupled residual (sin, cos, sinh): a per-entry bound against mpmath, derived in tests/blockcoupled_bound.py ----------------
import blockcoupled_bound as BB

# the storing launch k_f_blockcoupled_store takes every one of these shapes (lazy_blockcoupled_launch: dense blocks of up to 64 rows, block
# bandwidths (1, 1), a verified colouring), odd blocks included
BC_STORES = {(1, 2): 1, (3, 32): 1, (5, 32): 1, (9, 64): 1, (7, 3): 1, (70, 2): 1}
BC_ASSERTED = {"k_f_blockcoupled_store": 0, "hand-over": 0}


@pytest.mark.parametrize("mode", ["store", "handover"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", BB.SHAPES, ids=["%dx%d" % s for s in BB.SHAPES])
def test_blockcoupled_complex_step_within_the_per_entry_bound(monkeypatch, shape, dtype, mode):
    nb, bs = shape
    monkeypatch.setenv("FDJAC_SMALL", "0")
    monkeypatch.setenv("FDJAC_LAZY_STORE", "1" if mode == "store" else "0")
    lay = BB.layout(nb, bs)
    colors = lay.colors()
    C = int(colors.max())
    t = torch.float64 if dtype == np.float64 else torch.float32
    x = torch.as_tensor(BB.operands(nb, bs, dtype), device="cuda")
    Jb = fd.BlockBandedMatrix(None, lay)
    plan = fd.make_plan(Jb, Jb, colors, "complex", dtype=dtype)
    f = fd.BuiltinF("blockcoupled", nb, bs, dtype=dtype)
    if mode == "store":
        assert f.lazy_caps & fd.lib.LAZY_CAP_STORE
        plan.set_lazy(f)
    stored = plan.info(fd.lib.INFO_LAZY_STORE)
    assert stored == (BC_STORES[shape] if mode == "store" else 0), (shape, mode, stored)
    out = torch.full((plan.out_len(0),), float("nan"), dtype=t, device="cuda")
    plan.enable_timing(2)
    plan.jacobian(f, x, [out])
    torch.cuda.synchronize()
    perturbs = plan.timings()["perturb"]["launches"]
    plan.enable_timing(0)
    assert (perturbs == 0) if stored else (perturbs >= 1 or mode == "store"), (shape, mode, perturbs)
    assert X.same_bits(plan.epsilons().astype(dtype), X.complex_epsilons(C, dtype)).all()
    ratio, at = BB.worst_ratio(lay.to_dense(out.cpu().numpy()), nb, bs, dtype)
    print("\nblock-coupled %s, %s %s: worst error / bound = %.4f at %s" % (mode, shape, np.dtype(dtype).name, ratio, at))
    assert ratio <= 1.0, (shape, mode, ratio, at)
    BC_ASSERTED["k_f_blockcoupled_store" if stored else "hand-over"] += 1


def test_blockcoupled_routes_were_asserted():
    print("\nblock-coupled routes asserted:", BC_ASSERTED)
    if sum(BC_ASSERTED.values()) == 4 * len(BB.SHAPES):
        assert BC_ASSERTED["k_f_blockcoupled_store"] == 2 * sum(BC_STORES.values()) and BC_ASSERTED["hand-over"] > 0
