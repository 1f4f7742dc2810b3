"""The STORING routes of general CSC patterns against the exact host model (tests/exact_model.py), bit for bit, on the operand matrix of
tests/test_gpu_exact_model.py: fd_csc_store_cols, fd_csc_store_cols_win, fd_csc_store_rows, fd_csc_store_ents (include/fdjac_device.h),
the 7-point column kernel k_f_lap7_store_cols, a runtime-compiled row functor (SparseRows below: SparseF::row restated from device
pointers to the pattern by rows) and a runtime-compiled separable-terms functor (SPARSE_TERMS of tests/test_gpu_jit.py).  The cases
live in tests/exact_store_cases.py (pure numpy; tests/test_exact_model.py evaluates every one with the model alone, checks the finite
share and that the division's fall-back rules are reached).  Every case asserts which kernel ran: FD_INFO_STORE_LAUNCH, the plan's
report of its last column-store launch, and -- for the row-wise routes -- the functor's own count of row-wise launches, which must
have grown on the very call whose output is compared.

THE SIGN OF AN UNPERTURBED ZERO.  Three forms of an unperturbed coordinate x_i of a colour's point are in play:
    the model (Julia's x + eps * false)      plus side x_i + copysign(0, eps_c), minus side x_i - copysign(0, eps_c)
    the hand-over path (k_perturb,           plus side x_i + (+0.0) whatever the sign of eps_c, minus side x_i - (+0.0) = x_i
      csrc/fdjac_kernels.hip: e0 = hit ? e : 0.0; v0 + e0, v0 - e0)
    the column kernels (fd_colour_point,     plus side v + (T)0, minus side v, f(x) from v: the hand-over path's operands exactly
      fd_column_point, fd_window_column_point)
They differ only at x_i = -0.0, and only for a forward difference with dir = -1: the model keeps -0.0 (-0.0 + -0.0), the library's
paths all form +0.0.  For dir = +1 and for central differences (eps_c > 0) model and library agree: +0.0 on the plus side, -0.0 on the
minus side and in f(x).  The row-wise kernels (fd_csc_store_rows, fd_csc_store_ents) took the plain term of x_i ITSELF on both sides
-- the operand of the minus side where the column kernels and the hand-over path use x_i + 0.0 on the plus side.
Which stored bits can differ:
  * the sparse row, SparseRows and SPARSE_TERMS: NONE, against the model or between routes.  The one term is w (v + (q v) v).  For
    v = -0.0: q v = -0.0, (q v) v = +0.0, v + +0.0 = +0.0, w (+0.0) = +0.0 -- and for v = +0.0 the same +0.0: the term does not see the
    sign of a zero coordinate, so every row value, numerator and quotient is the same whichever zero the point holds.
  * the 7-point row ((((((d + s) + w) + e) + n) + u) - 6 c) + (c c) e: none at any operand of these cases.  A sum's value depends on
    the sign of a zero operand only while EVERY operand so far is a zero (z + b = b for b != 0, and an exact cancellation gives +0.0
    whatever zeros came before).  The row of a stored entry (r, j) reads the perturbed coordinate x_j + eps_c; unless that is exactly
    0 (x_j = -eps_c) the chain holds a non-zero operand from there on, (c c) e is added to a non-zero sum, and the row value is the
    same.  With x_j = -eps_c, every other coordinate of the row a zero and the caller's f_in a zero in that row, the stored zero's sign
    could differ from the model's for dir = -1 -- no case has x_j = -eps_c (checked per case below).
  * a functor that SEES the sign of a zero (w / v, copysign): between the library's routes the row-wise kernels were the odd ones out
    -- for every direction: their plus side summed term(-0.0) where the column kernels and the hand-over path sum term(+0.0).  SIGN_TERMS
    below (term = v + copysign(1, v)) shows it; test_sign_sensitive_terms_store_the_same_bits_on_every_route holds the hand-over path,
    the column store, fd_csc_store_rows and fd_csc_store_ents to one numpy evaluation of the library's point (x_i + 0.0 / x_i).  The
    row-wise kernels now send a row that reads a -0.0 through fd_csc_rows_signed_zero (include/fdjac_device.h).  Against the MODEL such a
    functor still differs on every route for dir = -1 (+0.0 against the reference's -0.0): that is the hand-over path's own form, which
    this module does not change.
So the signed_zeros / dir = -1 cases PIN bit equality with the model on every route for the residuals the library ships."""
import struct

import numpy as np
import pytest

import exact_model as X
import exact_store_cases as S
import hess_model
from test_gpu_exact_model import _check
from test_gpu_jit import SPARSE_TERMS
import finitediff_jl_amd as fd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SPARSE_ROWS = """
// FD_F_SPARSE's row (csrc/fdjac_functor_f.hip, SparseF::row) from device pointers to the pattern by rows: the entries (r, j) of row r,
// ascending j, left to right, w(r, j) * (v + (v / 4) v) with w = 1 + ((r + 3 j) mod 8) / 8; the first term is assigned.  Generic in the
// point's value type V (real_t for forward / central differences, fd_cplx<real_t> for the complex step: tests/test_gpu_exact_complex.py)
struct SparseRows {
    const long long *rp;
    const int *rc;
    template <class P> __device__ typename P::value_type operator()(long long r, const P &X) const
    {
        typedef typename P::value_type V;
        const long long a = rp[r], b = rp[r + 1];
        V s = V{};
        for (long long k = a; k < b; ++k) {
            const long long j = rc[k];
            const V v = X(j);
            const V t = ((real_t)1 + (real_t)0.125 * (real_t)(int)((r + 3 * j) & 7)) * (v + ((real_t)0.25 * v) * v);
            s = k == a ? t : s + t;
        }
        return s;
    }
};
"""

SIGN_TERMS = """
// the smallest separable term that sees the sign of a zero coordinate: term(-0.0) = -1, term(+0.0) = +1
struct SignTerms {
    template <class T> __device__ T term(long long r, long long j, T v) const { return v + (T)__builtin_copysign(1.0, (double)v); }
};
"""

LAUNCH = {"none": fd.lib.STORE_LAUNCH_NONE, "cols": fd.lib.STORE_LAUNCH_COLS, "cols_win": fd.lib.STORE_LAUNCH_COLS_WIN,
          "rows": fd.lib.STORE_LAUNCH_ROWS, "ents": fd.lib.STORE_LAUNCH_ENTS, "family": fd.lib.STORE_LAUNCH_FAMILY}
ROW_WISE = ("rows", "ents", "terms", "terms_ents")
# what the module reports per route: the cases whose assertion that the route's kernel ran has passed
ASSERTED = {"plain column store": 0, "windowed column store": 0, "row-wise store": 0, "entry-parallel store": 0, "lap7 column kernel": 0,
            "JIT row functor": 0, "terms functor": 0}
RAN = []
COMPILED = {}      # the first functor of each compiled text and element type, kept: the library drops a module with its last functor


def _functor(case, inp, plan, keep):
    route, dtype = case["route"], inp["dtype"]
    M, N, colptr, rowval = (inp[k] for k in ("M", "N", "colptr", "rowval"))
    if route == "lap7":
        return fd.BuiltinF("lap7", *S.LAP7[case["pattern"]], dtype=dtype)
    if route == "jit":
        rp, rc = hess_model.rows_of(M, N, colptr - 1, rowval - 1)
        rp_d, rc_d = torch.as_tensor(rp, device="cuda"), torch.as_tensor(rc, device="cuda")
        keep += [rp_d, rc_d]
        f = fd.JitF(SPARSE_ROWS, "SparseRows", M, N, params=struct.pack("PP", rp_d.data_ptr(), rc_d.data_ptr()), dtype=dtype)
        COMPILED.setdefault(("rows", np.dtype(dtype).name), (f, rp_d, rc_d))
        return f
    if route in ("terms", "terms_ents"):
        f = fd.JitTerms(SPARSE_TERMS, "SparseTerms", plan)
        COMPILED.setdefault(("terms", np.dtype(dtype).name), f)
        return f
    return fd.BuiltinF.sparse(M, N, colptr, rowval, dtype=dtype)


def _row_stores(f):
    n = f.row_stores
    return n() if callable(n) else n


def _count(case, launch):
    route = case["route"]
    if route == "jit":
        ASSERTED["JIT row functor"] += 1
    elif route in ("terms", "terms_ents"):
        ASSERTED["terms functor"] += 1
    elif route == "lap7" and launch == "family":
        ASSERTED["lap7 column kernel"] += 1
    elif launch in ("cols", "cols_win", "rows", "ents"):
        ASSERTED[{"cols": "plain column store", "cols_win": "windowed column store", "rows": "row-wise store", "ents": "entry-parallel store"}[launch]] += 1


@pytest.mark.parametrize("case", S.CASES, ids=[c["id"] for c in S.CASES])
def test_store_route_against_the_model(monkeypatch, case):
    monkeypatch.setenv("FDJAC_SMALL", "0")            # the defined two-level order of the step-size reduction at every N
    monkeypatch.delenv("FDJAC_LAZY_STORE", raising=False)
    if case["route"] in ("ents", "terms_ents"):
        monkeypatch.setenv("FDJAC_ROWS_ENTS", "1")
    else:
        monkeypatch.delenv("FDJAC_ROWS_ENTS", raising=False)
    inp = S.inputs(case)
    M, N, colptr, rowval, colors, C, dtype = (inp[k] for k in ("M", "N", "colptr", "rowval", "colors", "C", "dtype"))
    fdtype, variant, route = case["fdtype"], case["variant"], case["route"]
    t = torch.float64 if dtype == np.float64 else torch.float32
    # no case sits on the one operand at which the 7-point row could see the sign of a zero (the head of this module)
    e_model, _ = X.epsilons(inp["x"], inp["c0"], C, fdtype, relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"], dtype=dtype)
    ok = (inp["c0"] >= 0) & np.isfinite(inp["x"])
    assert not (inp["x"][ok] == -e_model[inp["c0"][ok]]).any()
    kw = dict(store_csc=True, store_rows=route in ROW_WISE, dtype=dtype)
    nnz_local = rowval.size
    if variant == "chunked":        # room for two colours' points and values at a time
        rnd = lambda n: (n + 31) // 32 * 32
        kw["scratch_bytes"] = 2 * (2 if fdtype == "central" else 1) * np.dtype(dtype).itemsize * (rnd(N) + rnd(M)) + 4096
    if variant == "colwindow":
        kw["col_window"] = S.COL_WINDOW
        nnz_local = int(colptr[S.COL_WINDOW[1]] - colptr[S.COL_WINDOW[0]])
    parts = [None] if variant != "colorrange" else [(a, C if b is None else b) for a, b in S.COLOR_RANGES]
    J = fd.SparseMatrixCSC(M, N, colptr, rowval)
    x = torch.as_tensor(inp["x"], device="cuda")
    x_before = x.clone()
    f_in = None if inp["f_in"] is None else torch.as_tensor(inp["f_in"], device="cuda")
    f_in_before = None if f_in is None else f_in.clone()
    keep = []
    for part in parts:
        plan = fd.make_plan(J, J, colors, fdtype, **(kw if part is None else dict(kw, color_range=part)))
        f = _functor(case, inp, plan, keep)
        plan.set_lazy(f)
        assert plan.out_len(0) == nnz_local
        assert plan.info(fd.lib.INFO_LAZY_STORE) == 1 and plan.info(fd.lib.INFO_STORE_CSC) == nnz_local, case["id"]
        want = S.layout(case, inp, part)

        def want_checked(D):
            lay = want(D)
            if part is None:    # the comparison means something only while most of the values are finite (MIN_FINITE)
                assert np.isfinite(lay[0]).mean() >= S.MIN_FINITE, float(np.isfinite(lay[0]).mean())
            return lay
        # the row-wise store of the built-in family starts once its check of the plan's pattern has reached the host: the same operands
        # until it has, at most four calls; the first call (a column kernel stored) and the first row-wise call are both compared
        launches = []
        for it in range(4 if route in ("rows", "ents") else 1):
            out = (torch.zeros if part is not None else lambda *a, **k: torch.full(*a, float("nan"), **k))((nnz_local,), dtype=t, device="cuda")
            before = _row_stores(f) if route in ROW_WISE else 0
            plan.jacobian(f, x, [out], f_in=f_in, relstep=inp["rel"], absstep=inp["ab"], dir=case["dir"])
            torch.cuda.synchronize()
            launches.append(plan.info(fd.lib.INFO_STORE_LAUNCH))
            row_wise = route in ROW_WISE and _row_stores(f) > before
            if it == 0 or row_wise:
                _check(plan, [out], want_checked, inp["x"], inp["c0"], C, fdtype, inp["rel"], inp["ab"], case["dir"], dtype, inp["f"],
                       defined_order=C <= 8, f_in=inp["f_in"])
            assert torch.equal(x.view(torch.int64 if dtype == np.float64 else torch.int32), x_before.view(torch.int64 if dtype == np.float64 else torch.int32))
            if f_in is not None:
                assert torch.equal(f_in, f_in_before)             # read, not written
            if row_wise:
                break
        # which kernel ran
        assert launches[-1] == LAUNCH[case["launch"]], (case["id"], launches)
        if route in ROW_WISE:
            assert row_wise, (case["id"], launches)
        # (the first call: a column kernel stored, the check ran beside it; a chunked call launches once per chunk, and the later
        #  chunks of the first call already go row by row)
        if route in ("rows", "ents") and variant != "chunked":
            assert len(launches) >= 2 and launches[0] in (LAUNCH["cols_win"], LAUNCH["family"]), (case["id"], launches)
        if variant == "chunked":
            assert plan.info(fd.lib.INFO_NCHUNKS) > 1
        assert plan.info(fd.lib.INFO_NCOLORS) == C
    _count(case, case["launch"])
    RAN.append((case["id"], route, case["family"]))


def test_every_route_was_asserted():
    # the module's report: per route, the cases whose assertion that the route ran has passed (a run of a selection reports only)
    print("\nstore routes asserted:", ASSERTED)
    ran = {(route, fam) for _id, route, fam in RAN}
    assert sum(ASSERTED.values()) <= len(RAN)
    if len(RAN) == len(S.CASES):      # (the whole table ran in this process: every route, and every edge family on every route, has PASSED)
        assert all(n > 0 for n in ASSERTED.values()), ASSERTED
        for fam in S.DIV_FAMILIES + ["nan_inf"]:
            for route in ("cols", "win", "rows", "ents", "lap7", "jit", "terms"):
                assert (route, fam) in ran, (fam, route)


def _row_sums(M, rs, terms):
    """Row r: its terms added left to right (ascending column), the first one assigned; an empty row is +0."""
    cnt = np.bincount(rs, minlength=M)
    start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    out = np.zeros(M, terms.dtype)
    for k in range(int(cnt.max())):
        sel = np.nonzero(cnt > k)[0]
        out[sel] = terms[start[sel] + k] if k == 0 else out[sel] + terms[start[sel] + k]
    return out


@pytest.mark.parametrize("fdtype,dir", S.DIRS, ids=["forward", "forwardm", "central"])
@pytest.mark.parametrize("pname", ["random_band600", "ragged400", "rows12"])
def test_sign_sensitive_terms_store_the_same_bits_on_every_route(monkeypatch, pname, fdtype, dir):
    # SIGN_TERMS at signed zeros: the hand-over path, the column store, fd_csc_store_rows and fd_csc_store_ents against ONE numpy
    # evaluation of the library's point -- an unperturbed coordinate is x_i + 0.0 on the plus side, x_i on the minus side and in f(x)
    # (the head of this module).  random_band600: rows in registers; ragged400: a row of 40 entries (the loop form); rows12: tiles
    # beyond the staged run.  The operands must tell the two zeros apart: the evaluation with x_i itself on the plus side differs.
    monkeypatch.setenv("FDJAC_SMALL", "0")
    M, N, colptr, rowval = S.pattern(pname)
    colors = S.colouring(pname, "greedy")
    c0, C = colors - 1, int(colors.max())
    x, rel, ab = G_operands("signed_zeros", pname, colors, N)
    assert np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any()
    J = fd.SparseMatrixCSC(M, N, colptr, rowval)
    xd = torch.as_tensor(x, device="cuda")
    nan = lambda: torch.full((rowval.size,), float("nan"), dtype=torch.float64, device="cuda")
    got = {}
    eps = None
    for name, ents in (("rows", False), ("ents", True)):
        if ents:
            monkeypatch.setenv("FDJAC_ROWS_ENTS", "1")
        else:
            monkeypatch.delenv("FDJAC_ROWS_ENTS", raising=False)
        pr = fd.make_plan(J, J, colors, fdtype, store_rows=True)
        ft = fd.JitTerms(SIGN_TERMS, "SignTerms", pr)
        COMPILED.setdefault(("sign", "float64"), ft)
        pr.set_lazy(ft)
        out, before = nan(), ft.row_stores
        pr.jacobian(ft, xd, [out], dir=dir)
        torch.cuda.synchronize()
        assert ft.row_stores == before + 1
        # (rows12: a tile holds more than 2048 entries, the plan builds no entry lists -- the switch then leaves the row form)
        assert pr.info(fd.lib.INFO_STORE_LAUNCH) == (LAUNCH["ents"] if ents and pname != "rows12" else LAUNCH["rows"])
        got[name] = out.cpu().numpy()
        eps = pr.epsilons()
        if not ents:
            pc = fd.make_plan(J, J, colors, fdtype, store_csc=True)
            pc.set_lazy(ft)
            out = nan()
            pc.jacobian(ft, xd, [out], dir=dir)
            assert ft.row_stores == before + 1 and pc.info(fd.lib.INFO_STORE_LAUNCH) == LAUNCH["cols_win"]
            got["cols_win"] = out.cpu().numpy()
            po = fd.make_plan(J, J, colors, fdtype)
            out = nan()
            po.jacobian(ft, xd, [out], dir=dir)
            assert po.info(fd.lib.INFO_LAZY_STORE) == 0
            got["hand-over"] = out.cpu().numpy()
            assert np.array_equal(pc.epsilons(), eps) and np.array_equal(po.epsilons(), eps)
    cols = np.repeat(np.arange(N), np.diff(colptr))
    order = np.lexsort((cols, rowval - 1))
    rs, cs = (rowval - 1)[order], cols[order]
    F = lambda p: _row_sums(M, rs, p[cs] + np.copysign(1.0, p[cs]))

    def expect(plus_zero):
        D = np.empty((C, M))
        for c in range(C):
            e, m = eps[c], c0 == c
            xp = np.where(m, x + e, x + plus_zero if plus_zero is not None else x)
            D[c] = (F(xp) - F(x)) / e if fdtype == "forward" else (F(xp) - F(np.where(m, x - e, x))) / (2.0 * e)
        return X.to_csc(D, c0, colptr, rowval)
    want, other = expect(0.0), expect(None)
    assert not X.same_bits(want, other).all()                  # the case tells x_i + 0.0 from x_i
    for name, g in got.items():
        m = X.same_bits(g, want)
        assert m.all(), (name, int((~m).sum()), g[~m][:4].tolist(), want[~m][:4].tolist())


def G_operands(family, pname, colors, N):
    import exact_general as G
    return G.operands(family, pname, colors, np.float64, 7 * N + int(colors.max()), N=N)
