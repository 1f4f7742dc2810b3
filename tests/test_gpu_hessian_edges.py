"""The objective Hessian / gradient (csrc/fdjac_hessian.hip; fd_obj_rows, fd_hess_entries, fd_grad_cols) against the exact host model
(tests/hess_model.py) at the edges of the plan builder and of the operands: the cases of tests/hess_cases.py.  Every objective is the
list-driven functor ListRows on the pattern's own rows, so one compiled module serves every pattern.  The plan's pattern and counts
against the model's triples; every slot of the CSC, dense and banded destinations bit for bit (a NaN matches any NaN; +0.0 outside
P); the forward (dir = +-1) and central gradient; sentinel guards around every output, x unchanged, the same plan called again with
another x; the host-staging entry points; the C ABI's 4-byte and 0-based index inputs."""
import ctypes

import numpy as np
import pytest

import exact_model as X
import hess_cases as C
import hess_model as hm
import finitediff_jl_amd as fd
from finitediff_jl_amd import lib as L_
from finitediff_jl_amd import patterns as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -12345.5
GUARD = 37
FD_ERR_ARG = 1
_OBJ, _PLANS = {}, {}


def _objective(name):
    """(f, S) of a pattern: the rows of S on the device (kept alive here), the functor's two pointers as its params"""
    if name not in _OBJ:
        M, N, cp, rv = C.pattern(name)
        rp, rc = hm.rows_of(M, N, cp, rv)
        rp_d = torch.as_tensor(rp, device="cuda")
        rc_d = torch.as_tensor(np.concatenate([rc, np.zeros(1, np.int32)]), device="cuda")        # (never empty)
        f = fd.ObjectiveF(hm.LISTROWS_SRC, "ListRows", M, N, params=np.array([rp_d.data_ptr(), rc_d.data_ptr()], np.uint64).tobytes())
        _OBJ[name] = (f, fd.SparseMatrixCSC(M, N, cp + 1, rv + 1), rp_d, rc_d)
    return _OBJ[name][:2]


def _plan(name, dest, band=None):
    """one cache per pattern and destination for the whole file: every case after the first calls a plan that has run before"""
    key = (name, dest, band)
    if key not in _PLANS:
        S = _objective(name)[1]
        x = np.zeros(S.n)
        _PLANS[key] = fd.GradientCache(x, dest, S) if dest in ("forward", "central") else fd.HessianCache(x, S, dest=dest, band=band)
    return _PLANS[key]


def _guarded(a):
    """a device copy of `a` inside a sentinel-filled buffer, and the buffer's expected content"""
    a = np.asarray(a, np.float64).ravel()
    want = np.full(a.size + 2 * GUARD, SENTINEL)
    want[GUARD:GUARD + a.size] = a
    buf = torch.as_tensor(want, device="cuda")
    return buf, buf[GUARD:GUARD + a.size], want


def _check(buf, want, what):
    """the whole buffer -- guards and values -- holds `want`'s bits"""
    got = buf.cpu().numpy() if not isinstance(buf, np.ndarray) else buf
    same = X.same_bits(got, want)
    bad = np.flatnonzero(~same)
    assert same.all(), (what, "%d of %d differ, first at %d (guard = %d): got %r, want %r" %
                        (bad.size, want.size - 2 * GUARD, bad[0] - GUARD, GUARD, got[bad[0]], want[bad[0]]))


def _expected(name, dest, band, i, j, h):
    """the destination's whole content from the model's upper entries: both slots of every entry, +0.0 everywhere else"""
    M, N, cp, rv = C.pattern(name)
    if dest == "csc":
        Pm = P.hessian_sparsity(_objective(name)[1])
        pcol = np.repeat(np.arange(N, dtype=np.int64), np.diff(Pm.colptr))
        key = pcol * N + (Pm.rowval - 1)                       # ascending: column-major, rows ascending
        out = np.full(key.size, np.nan)
        up, lo = np.searchsorted(key, j * N + i), np.searchsorted(key, i * N + j)
        assert np.array_equal(key[up], j * N + i) and np.array_equal(key[lo], i * N + j) and np.unique(np.concatenate([up, lo])).size == key.size
    elif dest == "banded":
        w = 2 * band + 1
        out = np.zeros(w * N)
        up, lo = (band + i - j) + w * j, (band + j - i) + w * i
    else:
        out = np.zeros(N * N)
        up, lo = i + j * N, j + i * N
    out[up] = h
    out[lo] = h
    return out


def _bands(name):
    N, bw = C.pattern(name)[1], C.plan_counts(name)["bandwidth"]
    return sorted({b for b in (bw, bw + 1, N - 1) if bw <= b < N})


def _steps(kw):
    return dict(relstep=kw[0], absstep=kw[1])


# ---- 1. the plan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.PATTERN_NAMES)
def test_plan_pattern_and_counts_are_the_models(name):
    M, N, cp, rv = C.pattern(name)
    f, S = _objective(name)
    want = P.hessian_sparsity(S)
    counts = C.plan_counts(name)
    for dest, band in [("csc", None), ("dense", None)] + [("banded", b) for b in _bands(name)]:
        cache = fd.HessianCache(np.zeros(N), S, dest=dest, band=band)
        Pm = cache.pattern()
        assert np.array_equal(Pm.colptr, want.colptr) and np.array_equal(Pm.rowval, want.rowval), dest
        got = {k: cache.info(getattr(L_, "HESS_INFO_" + k.upper())) for k in ("upper", "nnz", "list_len", "bandwidth")}
        assert got == counts, (dest, got, counts)
        out_len = {"csc": counts["nnz"], "dense": N * N}.get(dest, (2 * (band or 0) + 1) * N)
        assert cache.info(L_.HESS_INFO_OUT_LEN) == out_len
    bw = counts["bandwidth"]
    for band in ([bw - 1] if bw else []) + [N, N + 3]:             # narrower than P, or not below N: refused
        with pytest.raises(L_.FdError) as e:
            fd.HessianCache(np.zeros(N), S, dest="banded", band=band)
        assert e.value.code == FD_ERR_ARG, band


def test_duplicated_and_unsorted_rowval_give_the_clean_plan_and_bits():
    name = "ragged_wide"
    M, N, cp, rv = C.pattern(name)
    f, S = _objective(name)
    dcp, drv = C.dup_unsorted(name)
    assert drv.size > rv.size and any(np.any(np.diff(drv[dcp[k]:dcp[k + 1]]) <= 0) for k in range(N))
    dirty = fd.SparseMatrixCSC(M, N, dcp + 1, drv + 1)
    clean_c, dirty_c = _plan(name, "csc"), fd.HessianCache(np.zeros(N), dirty, dest="csc")
    Pc, Pd = clean_c.pattern(), dirty_c.pattern()
    assert np.array_equal(Pc.colptr, Pd.colptr) and np.array_equal(Pc.rowval, Pd.rowval)
    for k in (L_.HESS_INFO_NNZ, L_.HESS_INFO_UPPER, L_.HESS_INFO_LIST_LEN, L_.HESS_INFO_BANDWIDTH):
        assert clean_c.info(k) == dirty_c.info(k), k
    m, op = C.model(name, "ordinary"), C.operands(name, "ordinary")
    want = _expected(name, "csc", None, *m["ij"], m["H"])
    xd = torch.as_tensor(np.array(op["x"]), device="cuda")
    buf, nz, full = _guarded(np.full(want.size, np.nan))
    full[GUARD:GUARD + want.size] = want
    fd.finite_difference_hessian_b(nz, f, xd, dirty_c)
    _check(buf, full, "csc")
    for fdtype, key in (("forward", ("forward", 1.0)), ("central", "central")):
        buf, g, full = _guarded(np.full(N, np.nan))
        full[GUARD:GUARD + N] = m[key]
        fd.finite_difference_gradient_b(g, f, xd, fd.GradientCache(np.zeros(N), fdtype, dirty))
        _check(buf, full, fdtype)


# ---- 2. every case against the model ---------------------------------------------------------------------------------------------------
def _run_case(name, family, x, m, op, all_dests):
    M, N, cp, rv = C.pattern(name)
    f, S = _objective(name)
    i, j = m["ij"]
    xbuf, xd, xfull = _guarded(x)
    dests = [("csc", None), ("banded", _bands(name)[0])]
    if all_dests:
        dests += [("dense", None)] + [("banded", b) for b in _bands(name)[1:]]
    for dest, band in dests:
        want = _expected(name, dest, band, i, j, m["H"])
        buf, H, full = _guarded(np.full(want.size, np.nan))
        full[GUARD:GUARD + want.size] = want
        fd.finite_difference_hessian_b(H, f, xd, _plan(name, dest, band), **_steps(op["hess"]))
        _check(buf, full, (name, family, dest, band))
    for fdtype, keys in (("forward", [("forward", d) for d in op["dirs"]]), ("central", ["central"])):
        for key in keys:
            buf, g, full = _guarded(np.full(N, np.nan))
            full[GUARD:GUARD + N] = m[key]
            fd.finite_difference_gradient_b(g, f, xd, _plan(name, fdtype), dir=key[1] if fdtype == "forward" else 1.0, **_steps(op["grad"]))
            _check(buf, full, (name, family, key))
    _check(xbuf, xfull, (name, family, "x"))                       # x and its surroundings: untouched


@pytest.mark.parametrize("case", C.CASES, ids=["%s-%s" % c for c in C.CASES])
def test_hessian_and_gradient_against_the_exact_model(case):
    name, family = case
    m, op = C.model(name, family), C.operands(name, family)
    fin = [np.isfinite(v).mean() for k, v in m.items() if k != "ij" and v.size]
    assert min(fin) >= C.MIN_FINITE, fin                           # (tests/test_hessian_cpu.py checks this for every case)
    # every destination and band for the ordinary operands; CSC and the narrowest band for the other families of a large pattern
    _run_case(name, family, op["x"], m, op, all_dests=family == "ordinary" or C.pattern(name)[1] <= 300)


@pytest.mark.parametrize("name", ["gaps", "dense_col", "chain_2049", "tiny_3_dense"])
def test_a_plan_called_again_with_another_x_returns_the_first_bits(name):
    M, N, cp, rv = C.pattern(name)
    f, S = _objective(name)
    phi = hm.phi_listrows(*hm.rows_of(M, N, cp, rv))
    x1, x2 = C.operands(name, "ordinary")["x"], C.second_x(name)
    m1 = C.model(name, "ordinary")
    i, j, h2 = hm.hessian_entries(phi, x2, M, N, cp, rv)
    g2 = hm.gradient(phi, x2, M, N, "forward", cp, rv)
    assert not X.same_bits(h2, m1["H"]).all()
    hc, gc = _plan(name, "csc"), _plan(name, "forward")
    for x, h, g in ((x1, m1["H"], m1["forward", 1.0]), (x2, h2, g2), (x1, m1["H"], m1["forward", 1.0])):
        xd = torch.as_tensor(np.array(x), device="cuda")
        want = _expected(name, "csc", None, i, j, h)
        buf, nz, full = _guarded(np.full(want.size, np.nan))
        full[GUARD:GUARD + want.size] = want
        gbuf, gd, gfull = _guarded(np.full(N, np.nan))
        gfull[GUARD:GUARD + N] = g
        fd.finite_difference_hessian_b(nz, f, xd, hc)               # (both reuse the plan's rows-pass scratch)
        fd.finite_difference_gradient_b(gd, f, xd, gc)
        _check(buf, full, "H")
        _check(gbuf, gfull, "g")


# ---- 3. host staging, and the pattern with no entries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gaps", "tiny_1", "tiny_2_dense", "tiny_2_diag", "tiny_3_dense", "tiny_3_diag"])
def test_host_staging_entry_points(name):
    M, N, cp, rv = C.pattern(name)
    f, S = _objective(name)
    m, op = C.model(name, "ordinary"), C.operands(name, "ordinary")
    x = op["x"].copy()
    for dest, band in [("csc", None), ("dense", None)] + [("banded", b) for b in _bands(name)]:
        want = _expected(name, dest, band, *m["ij"], m["H"])
        full = np.full(want.size + 2 * GUARD, SENTINEL)
        H = full[GUARD:GUARD + want.size]
        fd.finite_difference_hessian_b(H, f, x, fd.HessianCache(x, S, dest=dest, band=band))       # numpy x and H: fd_hessian
        ref = np.full(full.size, SENTINEL)
        ref[GUARD:GUARD + want.size] = want
        _check(full, ref, (dest, band))
    for fdtype, d, key in (("forward", 1.0, ("forward", 1.0)), ("forward", -1.0, ("forward", -1.0)), ("central", 1.0, "central")):
        full = np.full(N + 2 * GUARD, SENTINEL)
        fd.finite_difference_gradient_b(full[GUARD:GUARD + N], f, x, fd.GradientCache(x, fdtype, S), dir=d)
        ref = np.full(full.size, SENTINEL)
        ref[GUARD:GUARD + N] = m[key]
        _check(full, ref, key)
    assert X.same_bits(x, op["x"]).all()


def test_a_pattern_with_no_entries_is_zero_without_a_launch():
    name = "empty"
    M, N, cp, rv = C.pattern(name)
    f, S = _objective(name)
    x = C.operands(name, "ordinary")["x"].copy()
    xd = torch.as_tensor(np.array(x), device="cuda")
    assert C.plan_counts(name)["upper"] == 0
    for dest, band, n in (("csc", None, 0), ("dense", None, N * N), ("banded", 0, N), ("banded", N - 1, (2 * N - 1) * N)):
        cache = fd.HessianCache(x, S, dest=dest, band=band)
        assert cache.info(L_.HESS_INFO_UPPER) == 0 and cache.info(L_.HESS_INFO_NNZ) == 0 and cache.info(L_.HESS_INFO_OUT_LEN) == n
        before = f.launches
        buf, H, full = _guarded(np.full(n, np.nan))
        full[GUARD:GUARD + n] = 0.0
        fd.finite_difference_hessian_b(H, f, xd, cache)               # device arrays
        _check(buf, full, dest)
        host = np.full(n + 2 * GUARD, SENTINEL)
        fd.finite_difference_hessian_b(host[GUARD:GUARD + n], f, x, cache)     # host arrays
        _check(host, full, dest)
        assert f.launches == before, dest


# ---- 4. the C ABI's index inputs api.py never sends ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_wide", "ragged_tall"])
def test_raw_abi_index_widths_and_bases(name):
    M, N, cp, rv = C.pattern(name)
    f, S = _objective(name)
    L = f.L
    ref = _plan(name, "csc")
    Pr = ref.pattern()
    m, op = C.model(name, "ordinary"), C.operands(name, "ordinary")
    want = _expected(name, "csc", None, *m["ij"], m["H"])
    xd = torch.as_tensor(np.array(op["x"]), device="cuda")
    for idx_bytes, idx_base in ((4, 0), (8, 0), (4, 1)):
        t = np.int32 if idx_bytes == 4 else np.int64
        cpa, rva = np.ascontiguousarray(cp + idx_base, t), np.ascontiguousarray(rv + idx_base, t)
        h = ctypes.c_void_p()
        L_.check(L.fd_hess_plan_create(f.ctx.handle, M, N, cpa.ctypes.data, rva.ctypes.data, idx_bytes, idx_base, L_.HESS_CSC, 0, ctypes.byref(h)))
        try:
            v = ctypes.c_int64()
            for k in (L_.HESS_INFO_NNZ, L_.HESS_INFO_UPPER, L_.HESS_INFO_LIST_LEN, L_.HESS_INFO_BANDWIDTH):
                L_.check(L.fd_hess_plan_info(h, k, ctypes.byref(v)))
                assert v.value == ref.info(k), (idx_bytes, idx_base, k)
            pcp, prv = np.full(N + 1, -1, np.int64), np.full(Pr.rowval.size, -1, np.int64)
            L_.check(L.fd_hess_plan_pattern(h, pcp.ctypes.data, prv.ctypes.data))
            assert np.array_equal(pcp + 1, Pr.colptr) and np.array_equal(prv + 1, Pr.rowval), (idx_bytes, idx_base)
            buf, nz, full = _guarded(np.full(want.size, np.nan))
            full[GUARD:GUARD + want.size] = want
            L_.check(L.fd_hessian_async(h, f.handle, xd.data_ptr(), -1.0, -1.0, nz.data_ptr()))
            _check(buf, full, (idx_bytes, idx_base))
        finally:
            L_.check(L.fd_hess_plan_destroy(h))
