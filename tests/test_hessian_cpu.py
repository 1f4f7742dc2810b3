"""CPU checks of the objective Hessian / gradient: the Hessian pattern P = pattern(S^T S) against scipy, the host exact model against an
independent restatement of the reference's loops (M = 1: bit for bit), and the new C ABI symbols (declared, exported, and failing
loudly without a GPU)."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P

import exact_model as X
import hess_cases as HC
import hess_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_objective_compile", "fd_objective_destroy", "fd_objective_counts", "fd_hess_plan_create", "fd_hess_plan_destroy",
               "fd_hess_plan_info", "fd_hess_plan_pattern", "fd_hessian_async", "fd_hessian", "fd_gradient_async", "fd_gradient")


def _scipy_pattern(M, N, colptr0, rowval0):
    S = sp.csc_matrix((np.ones(rowval0.size), rowval0, colptr0), shape=(M, N))
    H = ((S.T @ S) != 0).tocsc()
    H.sort_indices()
    return H.indptr.astype(np.int64), H.indices.astype(np.int64)


def _supports():
    n = 9
    cp, rv = P.tridiag_csc(n)
    yield "tridiagonal", n, n, cp - 1, rv - 1
    cp, rv = P.lap5_csc(6, 5)
    yield "5-point grid", 30, 30, cp - 1, rv - 1
    M, N = 40, 23
    cp, rv = hm.randrows_support(M, N, N - 4)
    yield "random rectangular", M, N, cp, rv
    yield "dense M = 1", 1, 8, np.arange(9, dtype=np.int64), np.zeros(8, np.int64)


@pytest.mark.parametrize("case", list(_supports()), ids=lambda c: c[0])
def test_hessian_sparsity_is_the_pattern_of_StS(case):
    name, M, N, cp, rv = case
    got = P.hessian_sparsity(fd.SparseMatrixCSC(M, N, cp + 1, rv + 1))
    want_cp, want_rv = _scipy_pattern(M, N, cp, rv)
    assert (got.m, got.n) == (N, N)
    assert np.array_equal(got.colptr - 1, want_cp) and np.array_equal(got.rowval - 1, want_rv), name
    if name == "random rectangular":
        assert M != N and (np.diff(cp) == 0).any()          # some columns no row reads: no diagonal there
        assert (np.diff(got.colptr) == 0).sum() == (np.diff(cp) == 0).sum()


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("n", [2, 7, 16])
@pytest.mark.parametrize("steps", [(None, None), (1e-3, 1e-5), (3e-5, -1.0)], ids=["default", "custom", "absstep=relstep"])
def test_model_is_the_reference_hessian_bit_for_bit_when_M_is_1(n, steps):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) * 3
    x[0] = 0.0                                   # the absstep branch
    x[-1] = -abs(x[-1])
    phi = hm.phi_polydiv(n)
    H, mask = hm.hessian(phi, x, 1, n, relstep=steps[0], absstep=steps[1])
    assert mask.all()
    assert _bits_equal(H, hm.ref_hessian(phi, x, relstep=steps[0], absstep=steps[1]))


@pytest.mark.parametrize("fdtype,dir", [("forward", 1.0), ("forward", -1.0), ("central", 1.0)])
@pytest.mark.parametrize("n", [2, 7, 16])
def test_model_is_the_reference_gradient_bit_for_bit_when_M_is_1(n, fdtype, dir):
    rng = np.random.default_rng(100 + n)
    x = rng.standard_normal(n)
    x[n // 2] = 0.0
    phi = hm.phi_polydiv(n)
    for relstep, absstep in ((None, None), (1e-4, 1e-7)):
        g = hm.gradient(phi, x, 1, n, fdtype, relstep=relstep, absstep=absstep, dir=dir)
        assert _bits_equal(g, hm.ref_gradient(phi, x, fdtype, relstep=relstep, absstep=absstep, dir=dir))


def test_model_sparse_sums_agree_with_the_dense_reference_to_rounding():
    # M > 1: per-row sums, equal in exact arithmetic to differencing the whole f -- and exact zeros off the pattern
    n = 40
    x = np.random.default_rng(3).standard_normal(n)
    cp, rv = hm.chain_support(n)
    H, mask = hm.hessian(hm.phi_chain(n), x, n, n, cp, rv)
    whole = hm.phi_chain(n)

    def f0(r, get):                              # f = sum_r phi_r as ONE row, for the restatement
        s = np.zeros(np.shape(r))
        for k in range(n):
            s = s + whole(np.full(np.shape(r), k, np.int64), get)
        return s
    R = hm.ref_hessian(f0, x)
    assert np.all(H[~mask] == 0) and not np.signbit(H[~mask]).any()
    assert np.max(np.abs(H - R)) <= 1e-4 * np.max(np.abs(R))


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    declared = set(re.findall(r"^(?:int|void \*|const char \*)\s*(fd(?:32)?_[a-z0-9_]+)\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in fd.lib.EXPORTS, name
        assert "fd32_" + name[3:] not in declared                  # Float64 only
    fd.lib.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", fd.lib.SO_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (fd(?:32)?_[a-z0-9_]+)", syms))
    assert set(NEW_SYMBOLS) <= exported


def test_new_entry_points_fail_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    fd.lib.build()
    L = fd.lib.load()
    h = C.c_void_p()
    n = C.c_int64()
    x = np.zeros(4)
    calls = {
        "fd_objective_compile": lambda: L.fd_objective_compile(None, b"struct F {};", b"F", None, 0, 1, 4, C.byref(h)),
        "fd_objective_destroy": lambda: L.fd_objective_destroy(None),
        "fd_objective_counts": lambda: L.fd_objective_counts(None, C.byref(n)),
        "fd_hess_plan_create": lambda: L.fd_hess_plan_create(None, 1, 4, None, None, 8, 1, 0, 0, C.byref(h)),
        "fd_hess_plan_destroy": lambda: L.fd_hess_plan_destroy(None),
        "fd_hess_plan_info": lambda: L.fd_hess_plan_info(None, 0, C.byref(n)),
        "fd_hess_plan_pattern": lambda: L.fd_hess_plan_pattern(None, None, None),
        "fd_hessian_async": lambda: L.fd_hessian_async(None, None, x.ctypes.data, -1.0, -1.0, x.ctypes.data),
        "fd_hessian": lambda: L.fd_hessian(None, None, x.ctypes.data, 0, -1.0, -1.0, x.ctypes.data, 0),
        "fd_gradient_async": lambda: L.fd_gradient_async(None, None, x.ctypes.data, 0, -1.0, -1.0, 1.0, x.ctypes.data),
        "fd_gradient": lambda: L.fd_gradient(None, None, x.ctypes.data, 0, 0, -1.0, -1.0, 1.0, x.ctypes.data, 0),
    }
    assert set(calls) == set(NEW_SYMBOLS)
    for name, call in calls.items():
        assert call() == 7, name                                       # FD_ERR_NODEVICE
        assert b"no HIP device" in L.fd_last_error(), name
    with pytest.raises(RuntimeError):
        fd.ObjectiveF(hm.CHAIN_SRC, "Chain", 4, 4, params=np.int64(4).tobytes())
    with pytest.raises(RuntimeError):
        fd.HessianCache(x, fd.SparseMatrixCSC(4, 4, *P.tridiag_csc(4)))


# ---- the edge cases of tests/hess_cases.py (run on the device by tests/test_gpu_hessian_edges.py) -----------------------------------------
@pytest.mark.parametrize("name", HC.PATTERN_NAMES)
def test_edge_patterns_sparsity_and_counts(name):
    M, N, cp, rv = HC.pattern(name)
    assert cp[0] == 0 and cp[-1] == rv.size and (rv.size == 0 or (rv.min() >= 0 and rv.max() < M))
    assert all(np.all(np.diff(rv[cp[j]:cp[j + 1]]) > 0) for j in range(N))
    got = P.hessian_sparsity(fd.SparseMatrixCSC(M, N, cp + 1, rv + 1))
    want_cp, want_rv = _scipy_pattern(M, N, cp, rv)
    assert np.array_equal(got.colptr - 1, want_cp) and np.array_equal(got.rowval - 1, want_rv)
    # the counts the plan must report, by a loop over the rows
    rows = [[] for _ in range(M)]
    for j in range(N):
        for r in rv[cp[j]:cp[j + 1]]:
            rows[r].append(j)
    lists = collections.Counter((i, j) for cs in rows for a, i in enumerate(cs) for j in cs[a:])
    brute = dict(upper=len(lists), nnz=2 * len(lists) - sum(1 for i, j in lists if i == j), list_len=sum(lists.values()),
                 bandwidth=max([cs[-1] - cs[0] for cs in rows if cs], default=0))
    assert HC.plan_counts(name) == brute
    assert brute["nnz"] == want_rv.size
    r, i, j = HC.triples(name)
    assert r.size == brute["list_len"] and sorted(zip(j.tolist(), i.tolist(), r.tolist())) == list(zip(j.tolist(), i.tolist(), r.tolist()))


def test_edge_patterns_cross_the_edges_they_are_named_for():
    c = {n: HC.plan_counts(n) for n in HC.PATTERN_NAMES}
    unread = lambda n: np.flatnonzero(np.diff(HC.pattern(n)[2]) == 0)
    assert (c["tiny_1"]["upper"], c["empty"]["upper"], c["m1_sparse"]["upper"]) == (1, 0, 15)
    assert [c["dense_row_%d" % k]["upper"] for k in (2047, 2048, 2049)] == [2047, 2048, 2049] and c["dense_row"]["upper"] == 70 * 71 // 2
    g = unread("gaps")
    assert 0 in g and 256 in g and 52 <= g.size <= 70 and np.diff(HC.pattern("empty_rows")[2]).sum() > 0
    M, N, cp, rv = HC.pattern("empty_rows")
    assert np.setdiff1d(np.arange(M), rv).size >= M // 3
    M, N, cp, rv = HC.pattern("dense_col")
    assert np.diff(cp).max() == M == 513
    assert c["diag"]["bandwidth"] == 0 and c["diag"]["upper"] == 260 and unread("m1_sparse").size == 4
    for n in HC.CHAIN_SIZES:                      # diagonals and columns: n; entries: 3 n - 3
        assert c["chain_%d" % n]["upper"] == 3 * n - 3
    for M, N, _cp, _rv in (HC.pattern("ragged_wide"), HC.pattern("ragged_tall")):
        assert M != N
    dcp, drv = HC.dup_unsorted()
    M, N, cp, rv = HC.pattern("ragged_wide")
    scp, srv = hm.support(M, N, dcp, drv)
    assert drv.size > rv.size and np.array_equal(scp, cp) and np.array_equal(srv, rv)


@pytest.mark.parametrize("which", ["chain", "randrows"])
def test_listrows_is_the_formula_on_a_given_support(which):
    if which == "chain":                          # rows of 2 or 3 columns, evaluated directly
        M = N = 12
        cp, rv = hm.chain_support(N)
    else:                                         # RandRows' support: 1 to 6 columns per row
        M, N = 40, 23
        cp, rv = hm.randrows_support(M, N, N - 4)
    rp, rc = hm.rows_of(M, N, cp, rv)
    assert rp[-1] == rc.size == rv.size and rc.dtype == np.int32
    x = np.random.default_rng(8).standard_normal(N)
    x[3] = -0.0
    got = hm.phi_listrows(rp, rc)(np.arange(M), lambda k: x[k])
    for r in range(M):
        cols = [j for j in range(N) if r in rv[cp[j]:cp[j + 1]]]
        assert rc[rp[r]:rp[r + 1]].tolist() == cols
        s = np.float64(0.0)
        for t, c in enumerate(cols):
            a, b = x[c], x[cols[(t + 1) % len(cols)]]
            s = s + (a * b + 0.5 * a * a) / (2.0 + b * b)
        assert _bits_equal(got[r], s), r
    assert _bits_equal(hm.phi_listrows(np.zeros(3, np.int64), np.zeros(0, np.int32))(np.arange(2), lambda k: x[k]), np.zeros(2))


@pytest.mark.parametrize("name", ["ragged", "gaps", "dense_row"])
def test_model_on_edge_patterns_agrees_with_the_dense_reference_to_rounding(name):
    # n <= 70, ordinary operands: the whole-f loops of the reference on f = sum_r phi_r (the tolerance of
    # test_model_sparse_sums_agree_with_the_dense_reference_to_rounding)
    if name == "dense_row":
        M, N, cp, rv = HC.pattern(name)
    elif name == "gaps":
        N = M = 61
        M, N, cp, rv = HC._from_rows(M, N, HC._random_rows(M, N, 1, 4, 21, window=8, skip_cols=sorted(set(range(0, N, 5)) | {N - 1})))
    else:
        M, N, cp, rv = HC._from_rows(45, 64, HC._random_rows(45, 64, 0, 9, 24))
    phi = hm.phi_listrows(*hm.rows_of(M, N, cp, rv))
    x = np.random.default_rng(3).standard_normal(N)
    H, mask = hm.hessian(phi, x, M, N, cp, rv)

    def f0(r, get):
        s = np.zeros(np.shape(r))
        for k in range(M):
            s = s + phi(np.full(np.shape(r), k, np.int64), get)
        return s
    R = hm.ref_hessian(f0, x)
    assert np.all(H[~mask] == 0) and not np.signbit(H[~mask]).any()
    assert np.max(np.abs(H - R)) <= 1e-4 * np.max(np.abs(R))


def _values(m):
    return [v for k, v in m.items() if k != "ij"]


@pytest.mark.parametrize("case", HC.CASES, ids=["%s-%s" % c for c in HC.CASES])
def test_edge_cases_are_mostly_finite(case):
    m, op = HC.model(*case), HC.operands(*case)
    N = HC.pattern(case[0])[1]
    assert op["x"].shape == (N,) and all(v.shape == (N,) for v in _values(m)[1:])
    for v in _values(m):
        assert v.size == 0 or np.isfinite(v).mean() >= HC.MIN_FINITE, (case, np.isfinite(v).mean())


def test_edge_cases_cover_every_family_and_reach_their_edges():
    fams = collections.Counter(f for _, f in HC.CASES)
    pats = collections.Counter(n for n, _ in HC.CASES)
    assert set(fams) == set(HC.FAMILIES) and min(fams.values()) >= 6 and set(pats) == set(HC.PATTERN_NAMES)
    for name, fam in HC.CASES:
        M, N, cp, rv = HC.pattern(name)
        op, cols = HC.operands(name, fam), np.array(HC.special_columns(name, fam), np.int64)
        x, (rel, ab) = op["x"], hm._defaults(*op["hess"], hm.HESS_RELSTEP)
        if N > 100 and cols.size:                 # a long list, a column beside an unread one, the first and the last
            cand = HC._candidates(name)[:5]
            assert len(set(cand) & set(cols.tolist())) >= (2 if fam == "inf_nan" else 3), (name, fam)
        if fam == "tie":
            a = rel * np.abs(x[cols])
            assert (a == ab).any() and (cols.size < 3 or ((a > ab).any() and (a < ab).any()))
        elif fam == "signed_zeros":
            assert (x[cols] == 0).all() and np.signbit(x[cols]).any()
        elif fam == "neg_dir":
            assert (x < 0).all() and -1.0 in op["dirs"]
        elif fam == "absstep0":
            assert ab == 0.0 and (x[cols] == 0).all() and np.isnan(HC.model(name, fam)["central"][cols]).all()
        elif fam == "absorbed":
            e = hm.step(x[cols], rel, ab)
            assert (x[cols] + e == x[cols]).all() and (x[cols] - e == x[cols]).all() and (e > 0).all()
        elif fam == "huge":
            e = hm.step(x[cols], rel, ab)
            with np.errstate(over="ignore"):
                assert np.isinf(e * e).any() and (np.abs(x[cols]) >= 2.0 ** 400).all() and (np.abs(x[cols]) <= 2.0 ** 511).all()
        elif fam == "tiny":
            e = hm.step(x[cols], rel, ab)
            assert (e * e == 0).any() and (np.abs(x[cols]) <= 2.0 ** -511).all() and (e > 0).all()
        elif fam == "subnormal":
            assert (np.abs(x[cols]) < 2.0 ** -1022).all() and (x[cols] != 0).all()
        elif fam == "inf_nan":
            assert np.isnan(x[cols]).sum() == 1 and np.isposinf(x[cols]).sum() == 1 and np.isneginf(x[cols]).sum() == 1
    # the NaN sits on a column no row reads where the pattern has one: the only place Julia's max and C's fmax part
    assert np.isnan(HC.operands("gaps", "inf_nan")["x"][np.diff(HC.pattern("gaps")[2]) == 0]).any()


# ---- perturbed models: each fault must change the bits of some case ---------------------------------------------------------------------------
def _faulty(name, fam, fault):
    M, N, cp, rv = HC.pattern(name)
    phi = hm.phi_listrows(*hm.rows_of(M, N, cp, rv))
    op = HC.operands(name, fam)
    with np.errstate(all="ignore"):
        i, j, h = hm.hessian_entries(phi, op["x"], M, N, cp, rv, *op["hess"], fault=fault)
        out = dict(ij=(i, j), H=h)
        for d in op["dirs"]:
            out["forward", d] = hm.gradient(phi, op["x"], M, N, "forward", cp, rv, *op["grad"], dir=d, fault=fault)
        out["central"] = hm.gradient(phi, op["x"], M, N, "central", cp, rv, *op["grad"], fault=fault)
    return out


def _changed(a, b):
    if a["H"].shape != b["H"].shape or not (np.array_equal(a["ij"][0], b["ij"][0]) and np.array_equal(a["ij"][1], b["ij"][1])):
        return True
    return any(not X.same_bits(a[k], b[k]).all() for k in a if k != "ij")


_PERTURBED_CASES = [c for c in HC.CASES if HC.pattern(c[0])[1] <= 300]


@pytest.mark.parametrize("fault", hm.FAULTS)
def test_perturbed_models_change_some_case(fault):
    n = sum(_changed(HC.model(*c), _faulty(*c, fault)) for c in _PERTURBED_CASES)
    print("perturbed model %-11s changes %3d of %d cases" % (fault, n, len(_PERTURBED_CASES)))
    if fault == "vi_over_vj":
        # the override order of the point's two coordinates shows only when i == j with vi != vj: the diagonal and the gradient pass
        # vi == vj, an off-diagonal entry has i != j.  No input can tell the two apart.
        assert n == 0
    else:
        assert n >= 1, fault                      # (the counts: DESIGN section 7)
