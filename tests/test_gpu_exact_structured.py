"""The routes that write the STRUCTURED storages against the exact host model (tests/exact_model.py), bit for bit: step sizes and every
stored value (a NaN matches any NaN), canaries around the destination, and the route that ran.  The cases live in
tests/exact_structured_cases.py (pure numpy; tests/test_exact_structured_cpu.py checks the finite share, the division rule's sides, the
families' edges and the model mutations on the CPU).

  BandedMatrix data, band as CSC   hand-over (k_decompress_banded / the window kernel) and fd_band_store_cols<L, U> (BandF, BandSign)
  BlockBandedMatrix data           hand-over (k_decompress_colrange_wg: paired where every first row, row count and destination is even
                                   and the destination 16-byte aligned, else scalar) and fd_colrange_store_cols (BlockRat, BlockSign)
  BandedBlockBandedMatrix data     hand-over (k_decompress_bbb), fd_bbb_store_cols (GridNL) and k_f_stencil5_store_bbb (lap5, lap5_nl)

WHICH ROUTE RAN.  A storing launch leaves the f! stage without a launch (the plan's stage counters: it is recorded as the decompression
stage) and reports FD_INFO_LAZY_STORE = 1; the hand-over path evaluates f! in a stage of its own, behind k_perturb for a compiled
functor.  The functor's own launch count: 1 for a storing launch, 2 for a forward difference on column-range / BBB storage (one plain
evaluation of f(x) beside it).  Where the plan or the launcher declines -- a caller's f_in (the subtrahend is then the caller's: the
plan takes the hand-over path, which subtracts it as given), a non-cyclic or invalid colouring, a band or block-banded colouring with
columns left out, more than 8 cyclic colours on a BandedMatrix, l + u > 8, non-uniform BBB blocks -- the case says so (`store` False)
and the test asserts that the f! stage ran.  (fd_bbb_store_cols writes the zeros of a column without a colour itself and keeps the
launch.)  A plan whose columns ALL lack a colour zero-fills the destination and runs no route: the zeros are compared.

FOUND.  k_f_stencil5_store_bbb stored a constant 0 / eps in the four corner slots of a column (rows (i +- 1, j +- 1)); the model, the
hand-over path and fd_bbb_store_cols store the row's difference with itself over the step -- NaN where the row reads a NaN / Inf
coordinate: 58 of 10 800 values of bbb-40x30x1-lap5_nl-wide-store-forward-f64-nan_inf.  Fixed in csrc/fdjac_f_stencil5.hip.

WHAT THE LIBRARY HAS NO SWITCH FOR.  k_decompress_colrange_wg's paired form is chosen by the layout and the destination's alignment
alone and its tile order is fixed (reversed): the variant "scalar" reaches the scalar instantiation on an even layout through a
destination that is only 8-byte aligned; odd layouts reach it anyway.  Which instantiation ran is not reported and not asserted.

THE SIGN OF AN UNPERTURBED ZERO (tests/test_gpu_exact_store.py has the full argument).  The model forms x_i + copysign(0, eps_c), every
route of the library x_i + (+0.0): different only at x_i = -0.0 for dir = -1.  BandF's term w (v + (v / 4) v) is +0.0 for either zero;
GridNL starts every row from c c >= +0.0 and a sum that holds a +0.0 or a non-zero operand never becomes -0.0 again; BlockRat's
x_k tot_b could see it only through a block sum that is -0.0, i.e. a run of blocks of nothing but -0.0 -- the CPU suite shows that no
such case is in the table (test_the_two_forms_of_an_unperturbed_zero: the stored bits are the same under both forms).  So every
case of these fixtures is held to the MODEL.  BandSign and BlockSign do see the sign; their dir = -1 cases are held to the model
evaluated at the library's point, which is the hand-over path's own form and not changed here."""
import collections
import time

import numpy as np
import pytest

import exact_model as X
import exact_structured_cases as S
import jit_fixtures as JF
from test_gpu_exact_model import _ulps
import finitediff_jl_amd as fd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

COMPILED = {}       # the first functor of each compiled text and element type, kept: the library drops a module with its last functor
ASSERTED = collections.Counter()     # (layout, route that ran, element type, fixture) -> cases whose route assertion and comparison passed
SLOWEST = [0.0, ""]
PAD = 16
SOURCES = {"band": (JF.BANDF, "BandF"), "band_sign": (JF.BAND_SIGN, "BandSign"), "blockrat": (JF.BLOCK_RAT, "BlockRat"),
           "block_sign": (JF.BLOCK_SIGN, "BlockSign"), "grid": (JF.GRID_NL, "GridNL"), "ragged": (JF.RAGGED_GRID, "RaggedGrid")}


def _functor(case, inp, keep):
    name, dtype, N = case["fixture"], inp["dtype"], inp["N"]
    if name in ("lap5", "lap5_nl"):
        nx, ny, _r = case["shape"]
        return fd.BuiltinF(name, nx, ny, dtype=dtype)
    if name in ("band", "band_sign"):
        prm = JF.band_params(N, inp["l"], inp["u"])
    elif name == "grid" and case["shape"] != "ragged":
        prm = JF.grid_params(*case["shape"])
    else:
        bs, bl, bu = (np.array(S.RAGGED_GRID, np.int64), 1, 1) if case["layout"] == "bbb" else S.block_shape(case)
        off = torch.as_tensor(np.concatenate([[0], np.cumsum(bs)]).astype(np.int64), device="cuda")
        blk = torch.as_tensor(np.repeat(np.arange(bs.size), bs).astype(np.int32), device="cuda")
        keep += [off, blk]
        prm = JF.block_params(bs.size, off.data_ptr(), blk.data_ptr(), bl, bu)
        if case["layout"] == "bbb":
            name = "ragged"
    src, sname = SOURCES[name]
    f = fd.JitF(src, sname, N, N, params=prm, dtype=dtype)
    COMPILED.setdefault((name, np.dtype(dtype).name), (f, list(keep)))
    return f


def _launches(f):
    return f.launches if isinstance(f, fd.JitF) else f.counts()[0]


def _storage(case, inp):
    """(J, sparsity, number of stored values, plan options)."""
    layout, N = case["layout"], inp["N"]
    kw = {}
    if layout == "band":
        J = fd.BandedMatrix(None, N, inp["l"], inp["u"])
        n = (inp["l"] + inp["u"] + 1) * N
        if case["variant"] == "colwindow":
            a, b = S.col_window(case)
            kw["col_window"] = (a, b)
            n = (inp["l"] + inp["u"] + 1) * (b - a)
        return J, None, n, kw
    if layout == "bandcsc":
        J = fd.SparseMatrixCSC(N, N, inp["colptr"], inp["rowval"], None)
        return J, J, inp["rowval"].size, kw
    lay = inp["lay"]
    J = fd.BlockBandedMatrix(None, lay) if layout == "blocks" else fd.BandedBlockBandedMatrix(None, lay)
    if case["variant"] == "chunked":
        rnd = lambda v: (v + 31) // 32 * 32
        pts = 2 if case["fdtype"] != "forward" else 1
        kw["scratch_bytes"] = S.CHUNK_COLOURS * pts * np.dtype(inp["dtype"]).itemsize * 2 * rnd(N) + 4096
    return J, J, lay.data_len, kw


def _compare(plan, got, case, inp):
    T, C, c0, x = inp["dtype"], inp["C"], inp["c0"], inp["x"]
    got_eps = plan.epsilons().astype(T)
    if case["fdtype"] == "complex":
        eps = X.complex_epsilons(C, T)
        assert X.same_bits(got_eps, eps).all(), ("eps", got_eps, eps)
        D = X.colour_values_complex(inp["fc"], x, c0, C, got_eps)
    else:
        eps, scaled = X.epsilons(x, c0, C, case["fdtype"], relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"], dtype=T)
        plain = ~scaled
        if C <= 8:          # (the register reduction's defined order; more colours: the per-colour lists, 4 ulps -- tests/test_gpu_exact_model.py)
            ok = X.same_bits(got_eps[plain], eps[plain])
        else:
            fin = np.isfinite(eps[plain])
            ok = (np.isnan(got_eps[plain]) == np.isnan(eps[plain])) & (~fin | (_ulps(got_eps[plain], eps[plain]) <= 4))
        assert ok.all(), ("eps", case["id"], got_eps, eps)
        if scaled.any():
            assert (_ulps(got_eps[scaled], eps[scaled]) <= 4).all(), ("scaled eps", got_eps, eps)
        D = X.colour_values(inp["f"], x, c0, C, got_eps, case["fdtype"], f_in=inp["f_in"], zero="library" if S.library_zero(case) else "model")
    want = S.layout_fn(case, inp)(D)
    assert np.isfinite(want).mean() >= S.MIN_FINITE or case["colouring"] in ("invalid",), case["id"]
    m = X.same_bits(got, want)
    assert m.all(), (case["id"], int((~m).sum()), np.nonzero(~m)[0][:6].tolist(), got[~m][:6].tolist(), want[~m][:6].tolist())


def _run(monkeypatch, case):
    monkeypatch.setenv("FDJAC_SMALL", "0")            # the defined two-level order of the step-size reduction at every N
    monkeypatch.delenv("FDJAC_LAZY_STORE", raising=False)
    t0 = time.perf_counter()
    inp = S.inputs(case)
    dtype, fdtype, route = inp["dtype"], case["fdtype"], case["route"]
    t = torch.float64 if dtype == np.float64 else torch.float32
    it = torch.int64 if dtype == np.float64 else torch.int32
    keep = []
    J, sp, n, kw = _storage(case, inp)
    plan = fd.make_plan(J, sp, inp["colors"], fdtype, dtype=dtype, **kw)
    f = _functor(case, inp, keep)
    if route == "store":
        plan.set_lazy(f)
    assert plan.out_len(0) == n, (case["id"], plan.out_len(0), n)
    pad = PAD + (1 if case["variant"] == "scalar" else 0)      # (an odd pad: the destination is 8-byte aligned only)
    canary = 7.0e37 if dtype == np.float32 else 7.0e77
    buf = torch.full((n + 2 * pad,), canary, dtype=t, device="cuda")
    out = buf[pad:pad + n]
    out.fill_(float("nan"))
    x = torch.as_tensor(inp["x"], device="cuda")
    x_before = x.clone()
    f_in = None if inp["f_in"] is None else torch.as_tensor(inp["f_in"], device="cuda")
    f_in_before = None if f_in is None else f_in.clone()
    plan.enable_timing(2)
    n0 = _launches(f)
    plan.jacobian(f, x, [out], f_in=f_in, relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"])
    torch.cuda.synchronize()
    launches = _launches(f) - n0
    tm = plan.timings()
    plan.enable_timing(0)
    if inp["C"] == 0:   # (every column without a colour: the plan zero-fills the destination and no route runs -- the zeros are compared)
        assert tm["perturb"]["launches"] == 0 and tm["decompress"]["launches"] == 0 and plan.fcalls_last <= 1, case["id"]
        _compare(plan, out.cpu().numpy(), case, inp)
        ASSERTED[(case["layout"], "zero-fill", case["dtype"], case["fixture"])] += 1
        return 0.0
    # (a storing launch is recorded as the decompression stage and nothing runs in the f! stage; every hand-over form -- materialised
    #  points behind k_perturb, or a built-in launcher's lazy points -- evaluates f! in a stage of its own)
    stored = tm["f"]["launches"] == 0
    assert stored or isinstance(f, fd.BuiltinF) or tm["perturb"]["launches"] >= 1, case["id"]
    C, pts = inp["C"], 2 if fdtype == "central" else 1
    # ---- which route ran
    assert stored == case["store"], (case["id"], "storing launch" if stored else "hand-over", tm["f"], tm["perturb"], plan.info(fd.lib.INFO_LAZY_STORE))
    if stored:
        assert plan.info(fd.lib.INFO_LAZY_STORE) == 1, case["id"]
        base = 1 if (fdtype == "forward" and case["layout"] in ("blocks", "bbb") and isinstance(f, fd.JitF)) else 0
        if case["variant"] != "chunked" and isinstance(f, fd.JitF):
            assert launches == 1 + base, (case["id"], launches)
    elif route == "handover":
        assert plan.info(fd.lib.INFO_LAZY_STORE) == 0, case["id"]
    if case["variant"] == "chunked":
        assert plan.info(fd.lib.INFO_NCHUNKS) > 1, case["id"]
    assert plan.info(fd.lib.INFO_NCOLORS) == C
    want_calls = C * pts + (1 if (fdtype == "forward" and f_in is None) else 0)
    assert plan.fcalls_last == want_calls, (case["id"], plan.fcalls_last, want_calls)
    # ---- canaries, inputs untouched
    assert bool((buf[:pad] == canary).all()) and bool((buf[pad + n:] == canary).all()), case["id"]
    assert torch.equal(x.view(it), x_before.view(it))
    if f_in is not None:
        assert torch.equal(f_in.view(it), f_in_before.view(it))
    _compare(plan, out.cpu().numpy(), case, inp)
    kind = "store" if stored else "handover"
    ASSERTED[(case["layout"], kind, case["dtype"], case["fixture"])] += 1
    dt = time.perf_counter() - t0
    return dt


GROUPS = collections.OrderedDict()
for _c in S.CASES:
    GROUPS.setdefault((_c["layout"], _c["route"], _c["dtype"], "matrix" if _c["shape"] in S.MID.values() or _c["shape"] == S.NAN_BLOCKS else "shapes"),
                      []).append(_c)


@pytest.mark.parametrize("group", list(GROUPS), ids=["-".join(g) for g in GROUPS])
def test_structured_route_against_the_model(monkeypatch, group):
    t0 = time.perf_counter()
    for case in GROUPS[group]:
        _run(monkeypatch, case)
    dt = time.perf_counter() - t0
    print("\n%s: %d cases, %.2f s" % ("-".join(group), len(GROUPS[group]), dt))
    if dt > SLOWEST[0]:
        SLOWEST[:] = [dt, "-".join(group)]


def test_every_route_was_asserted():
    # the module's report: per (layout, route that RAN, element type, fixture), the cases whose route assertion and comparison passed
    print("\nstructured routes asserted:")
    for k in sorted(ASSERTED):
        print("   ", k, ASSERTED[k])
    print("slowest group: %s %.2f s" % (SLOWEST[1], SLOWEST[0]))
    assert sum(ASSERTED.values()) <= len(S.CASES)
    if sum(ASSERTED.values()) == len(S.CASES):       # (the whole table ran in this process)
        ran = {(k[0], k[1]) for k in ASSERTED}
        for layout in ("band", "blocks", "bbb"):
            assert (layout, "store") in ran and (layout, "handover") in ran, ran
        assert ("bandcsc", "store") in ran
        assert any(k[3] == "lap5_nl" and k[1] == "store" for k in ASSERTED)
        assert any(k[3] in ("band_sign", "block_sign") and k[1] == "store" for k in ASSERTED)
