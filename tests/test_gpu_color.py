"""fd_color_columns_device / fd_color_check_device on the GPU (csrc/fdjac_color.hip): the device's colour vector equals the host
model's (tests/color_model.py: greedy in order of descending priority) element for element, whatever the index width, the base, the
colour width and the schedule; validity at sizes the model is too slow for; the checker; the errors; and the whole route pattern on
the device -> colours -> plan -> Jacobian with nothing on the host."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P

import color_model as cm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

COMBOS = [(it, base, ct) for it in (np.int32, np.int64) for base in (0, 1) for ct in (torch.int32, torch.int64)]


def _to_dev(colptr, rowval, itype=np.int64, base=1):
    """1-based int64 host arrays -> device tensors of `itype`, `base`-based."""
    return (torch.as_tensor((colptr - (1 - base)).astype(itype), device="cuda"), torch.as_tensor((rowval - (1 - base)).astype(itype), device="cuda"))


def _empty_ends():
    colptr, rowval = P.tridiag_csc(50)
    rowval = rowval[colptr[1] - 1:colptr[-2] - 1]        # drop the entries of the first and the last column
    colptr = np.concatenate([[1], colptr[1:-1] - (colptr[1] - 1), [colptr[-2] - (colptr[1] - 1)]]).astype(np.int64)
    return colptr, rowval


CASES = {}
for _n in (1, 2, 3, 64, 65, 4097, 100_000):
    CASES["tridiagonal %d" % _n] = (lambda n=_n: (n, n) + tuple(P.tridiag_csc(n)))
CASES["5-point 23 x 17"] = lambda: (23 * 17, 23 * 17) + tuple(P.lap5_csc(23, 17))
CASES["5-point 300 x 200"] = lambda: (60_000, 60_000) + tuple(P.lap5_csc(300, 200))
for _s in (1, 2, 3):
    CASES["random band square seed %d" % _s] = (lambda s=_s: (30_000, 30_000) + tuple(cm.random_band(30_000, 30_000, 6, 300, s)))
    CASES["random band 20000 x 30000 seed %d" % _s] = (lambda s=_s: (20_000, 30_000) + tuple(cm.random_band(20_000, 30_000, 4, 50, s)))
CASES["random 40 x 60"] = lambda: (40, 60) + tuple(P.csc_from_dense(cm.random_40x60().astype(float)))
CASES["first and last column empty"] = lambda: (50, 50) + _empty_ends()
CASES["one column, no entries"] = lambda: (1, 1, np.array([1, 1], np.int64), np.empty(0, np.int64))


@functools.lru_cache(maxsize=None)
def _case(name):
    M, N, colptr, rowval = CASES[name]()
    return M, N, colptr, rowval, cm.greedy(M, N, colptr, rowval)


def _unchanged(t, a):
    return np.array_equal(t.cpu().numpy(), a)


@pytest.mark.parametrize("name", list(CASES))
def test_device_colours_equal_the_model_bit_for_bit(name):
    M, N, colptr, rowval, want = _case(name)
    empty = np.diff(colptr) == 0
    assert np.all(want[empty] == 1)
    if name == "first and last column empty":
        assert empty[0] and empty[-1] and not empty[1:-1].any()
    for itype, base, ctype in COMBOS:
        cp, rv = _to_dev(colptr, rowval, itype, base)
        cp0, rv0 = cp.cpu().numpy().copy(), rv.cpu().numpy().copy()
        colors, nc = fd.matrix_colors_device(M, N, cp, rv, idx_base=base, color_dtype=ctype)
        assert colors.dtype == ctype and colors.is_cuda and colors.numel() == N
        got = colors.cpu().numpy().astype(np.int64)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, itype.__name__, base, str(ctype), int(bad.size), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
        assert nc == int(want.max())
        assert _unchanged(cp, cp0) and _unchanged(rv, rv0)
        assert fd.check_colors_device(M, N, cp, rv, colors, idx_base=base) == 0


def test_dense_row_finishes_in_the_one_workgroup_tail():
    # 50 x 3000, row 1 dense: a clique of 3000 columns -- 3000 colours and 3000 dependency levels under ANY greedy order.  The levels
    # run inside one launch (csrc/fdjac_color.hip, k_col_tail).  The time limit is no speed claim: it only separates "returns" from
    # "a launch and a read-back per level, or a spin"; the other plan-time tests of this size set none, a minute is generous.
    M, N = 50, 3000
    colptr, rowval = cm.dense_row(M, N)
    want = cm.greedy(M, N, colptr, rowval)
    assert want.max() == N and np.array_equal(np.sort(want), np.arange(1, N + 1))
    cp, rv = _to_dev(colptr, rowval)
    t0 = time.perf_counter()
    colors, nc = fd.matrix_colors_device(M, N, cp, rv)
    dt = time.perf_counter() - t0
    print("dense row 50 x 3000: %d colours in %.3f s" % (nc, dt))
    assert nc == N and np.array_equal(colors.cpu().numpy().astype(np.int64), want)
    assert fd.check_colors_device(M, N, cp, rv, colors) == 0
    assert dt < 60.0


@pytest.mark.parametrize("name", ["random band square seed 1", "5-point 300 x 200", "dense row 40 x 700"])
def test_colours_do_not_depend_on_the_schedule(monkeypatch, name):
    if name.startswith("dense row"):
        M, N = 40, 700
        colptr, rowval = cm.dense_row(M, N, seed=5)
        want = cm.greedy(M, N, colptr, rowval)
    else:
        M, N, colptr, rowval, want = _case(name)
    cp, rv = _to_dev(colptr, rowval)
    runs = [fd.matrix_colors_device(M, N, cp, rv)[0] for _ in range(3)]
    # one round per read-back of the worklist length, and no one-workgroup tail: every level is a launch of the round kernel
    monkeypatch.setenv("FDJAC_COLOR_BATCH", "1")
    monkeypatch.setenv("FDJAC_COLOR_TAIL", "0")
    runs.append(fd.matrix_colors_device(M, N, cp, rv)[0])
    monkeypatch.setenv("FDJAC_COLOR_BATCH", "3")
    runs.append(fd.matrix_colors_device(M, N, cp, rv)[0])
    for r in runs:
        assert torch.equal(r, runs[0])
    assert np.array_equal(runs[0].cpu().numpy().astype(np.int64), want)


def _delta(M, N, colptr, rowval):
    """The largest number of conflicting columns of any column, from the pattern of A^T A (scipy)."""
    import scipy.sparse as sp
    A = sp.csc_matrix((np.ones(rowval.size, np.float32), (rowval - 1).astype(np.int64), (colptr - 1).astype(np.int64)), shape=(M, N))
    B = (A.T @ A).tocsc()
    B.setdiag(0)
    B.eliminate_zeros()
    return int(np.diff(B.indptr).max())


def _terms_probe_band(N):
    """The random band of scripts/terms_probe.py: 6 rows within +-300 of the diagonal per column, duplicates dropped."""
    rng = np.random.default_rng(1)
    offs = np.sort(rng.integers(-300, 301, size=(N, 6)), axis=1)
    rows = np.arange(N)[:, None] + offs
    keep = (rows >= 0) & (rows < N)
    keep[:, 1:] &= rows[:, 1:] != rows[:, :-1]
    colptr = np.empty(N + 1, np.int64)
    colptr[0] = 1
    np.cumsum(keep.sum(axis=1), out=colptr[1:])
    colptr[1:] += 1
    return colptr, (rows[keep] + 1).astype(np.int64)


@pytest.mark.parametrize("name", ["random band 2e6 x 6", "5-point 4000 x 2500"])
def test_valid_colouring_at_size(name):
    if name.startswith("random"):
        N = 2_000_000
        colptr, rowval = _terms_probe_band(N)
    else:
        N = 4000 * 2500
        colptr, rowval = P.lap5_csc(4000, 2500)
    cp, rv = _to_dev(colptr, rowval, np.int32, 1)
    colors, nc = fd.matrix_colors_device(N, N, cp, rv)
    delta = _delta(N, N, colptr, rowval)
    bad = fd.check_colors_device(N, N, cp, rv, colors)
    print("%s: %d colours on the device, Delta = %d, rows with a repeated colour: %d" % (name, nc, delta, bad))
    assert bad == 0
    assert int(colors.min()) >= 1 and int(colors.max()) == nc
    assert nc <= delta + 1          # the greedy bound, in any order
    if name.startswith("random"):   # recorded, not asserted: there is no derivable bound between two greedy orders
        host = fd.matrix_colors(fd.SparseMatrixCSC(N, N, colptr, rowval))
        print("%s: fd_color_columns_greedy (natural order) uses %d colours, the device (priority order) %d" % (name, int(host.max()), nc))


def test_the_checker_counts_the_rows_with_a_repeated_colour():
    M, N, colptr, rowval, want = _case("random band square seed 2")
    cp, rv = _to_dev(colptr, rowval, np.int32, 0)
    Cn = int(want.max())
    assert fd.check_colors_device(M, N, cp, rv, torch.as_tensor(want, device="cuda"), idx_base=0) == 0
    spoilt = want.copy()
    spoilt[::1001] = spoilt[::1001] % Cn + 1          # (the corruption tests/test_gpu_planbuild.py uses)
    n_bad = cm.bad_rows(M, colptr, rowval, spoilt)
    assert n_bad > 0
    for ctype in (np.int32, np.int64):
        assert fd.check_colors_device(M, N, cp, rv, torch.as_tensor(spoilt.astype(ctype), device="cuda"), idx_base=0) == n_bad
    # colour 0 = uncoloured: ignored
    holes = spoilt.copy()
    holes[::1001] = 0
    assert cm.bad_rows(M, colptr, rowval, holes) == 0
    assert fd.check_colors_device(M, N, cp, rv, torch.as_tensor(holes, device="cuda"), idx_base=0) == 0
    assert fd.check_colors_device(M, N, cp, rv, torch.zeros(N, dtype=torch.int32, device="cuda"), idx_base=0) == 0
    # a long row (the wavefront path of the checker) with one colour repeated, and colours far apart
    M2, N2 = 50, 3000
    colptr2, rowval2 = cm.dense_row(M2, N2)
    cp2, rv2 = _to_dev(colptr2, rowval2)
    c2 = np.arange(1, N2 + 1, dtype=np.int64) * 100_003
    assert fd.check_colors_device(M2, N2, cp2, rv2, torch.as_tensor(c2, device="cuda")) == 0
    c2[2999] = c2[17]
    assert cm.bad_rows(M2, colptr2, rowval2, c2) >= 1
    assert fd.check_colors_device(M2, N2, cp2, rv2, torch.as_tensor(c2, device="cuda")) == cm.bad_rows(M2, colptr2, rowval2, c2)


SPARSE_TERMS = """
struct SparseTerms {
    template <class T> __device__ T term(long long r, long long j, T v) const
    {
        return ((real_t)1 + (real_t)0.125 * (real_t)(int)((r + 3 * j) & 7)) * (v + ((real_t)0.25 * v) * v);
    }
};
"""


def _sparse_np(M, N, colptr, rowval):
    """The built-in sparse family restated in numpy (tests/test_gpu_jit.py): row r = sum over its columns, left to right."""
    cols = P.csc_cols(colptr) - 1
    rows = rowval - 1
    order = np.lexsort((cols, rows))
    rs, cs = rows[order], cols[order]
    cnt = np.bincount(rs, minlength=M)
    start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    maxlen = int(cnt.max()) if cnt.size else 0
    w = 1.0 + 0.125 * ((rs + 3 * cs) & 7)

    def f(fx, xx):
        t = w * (xx[cs] + (0.25 * xx[cs]) * xx[cs])
        out = np.zeros(M, dtype=xx.dtype)
        for k in range(maxlen):
            sel = np.nonzero(cnt > k)[0]
            out[sel] = t[start[sel] + k] if k == 0 else out[sel] + t[start[sel] + k]
        fx[:] = out
    return f


@pytest.mark.parametrize("fdtype", ["forward", "central"])
def test_pattern_to_jacobian_with_nothing_on_the_host(oracle, fdtype):
    N, seed = 5000, 4
    colptr, rowval = cm.random_band(N, N, 6, 300, seed)
    cp, rv = _to_dev(colptr, rowval, np.int32, 1)
    colors, nc = fd.matrix_colors_device(N, N, cp, rv)                      # the colours never leave the device on this route
    plan = fd.make_plan_csc_device(N, N, cp, rv, colors, fdtype)
    assert plan.info(fd.lib.INFO_NCOLORS) == nc
    x = np.random.default_rng(seed).random(N) + 0.1
    xd = torch.as_tensor(x, device="cuda")
    fb = fd.BuiltinF.sparse(N, N, colptr, rowval)
    got = torch.full((rowval.size,), float("nan"), dtype=torch.float64, device="cuda")
    plan.jacobian(fb, xd, [got])
    host_colors = colors.cpu().numpy().astype(np.int64)                     # copied back for the checker only
    assert cm.valid(N, colptr, rowval, host_colors)
    of = oracle.PyF(_sparse_np(N, N, colptr, rowval), N, N)
    want = oracle.jacobian(fdtype, of, x, host_colors, M=N, kind=oracle.PAT_CSC_COMMON, colptr=colptr, rowval=rowval)
    fs = max(float(np.abs(want["fx"]).max()) if "fx" in want else 60.0, 1.0)
    atol = 16 * np.finfo(np.float64).eps * fs / float(np.min(np.abs(plan.epsilons())))
    g = got.cpu().numpy()
    assert not np.isnan(g).any()
    assert np.all(np.abs(g - want["out"]) <= 1e-6 * np.abs(want["out"]) + atol)
    # a run-time compiled functor through the column store: the same bits whether the plan was built from the device colours or
    # from the same colours handed over as a host array
    J = fd.SparseMatrixCSC(N, N, colptr, rowval, None)
    ft = fd.JitTerms(SPARSE_TERMS, "SparseTerms", fd.make_plan(J, J, host_colors, fdtype, store_rows=True))
    outs, lazy = [], []
    for p in (fd.make_plan_csc_device(N, N, cp, rv, colors, fdtype, store_csc=True), fd.make_plan(J, J, host_colors, fdtype, store_csc=True)):
        p.set_lazy(ft)
        o = torch.full((rowval.size,), float("nan"), dtype=torch.float64, device="cuda")
        p.jacobian(ft, xd, [o])
        outs.append(o)
        lazy.append(p.info(fd.lib.INFO_LAZY_STORE))
    assert lazy == [1, 1]
    assert not torch.isnan(outs[0]).any() and torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))
    assert torch.equal(outs[0].view(torch.int64), got.view(torch.int64))


def test_errors_and_untouched_inputs():
    N = 20_000
    colptr, rowval = P.tridiag_csc(N)
    L = fd.lib.load()
    ctx = fd.Context.default()
    cp, rv = _to_dev(colptr, rowval)
    out = torch.zeros(N, dtype=torch.int32, device="cuda")
    # a row outside 1..M; a decreasing colptr: FD_ERR_SHAPE with a message, found on the device
    bad_rv = rv.clone()
    bad_rv[12345] = N + 7
    bad_cp = cp.clone()
    bad_cp[777] = bad_cp[776] - 1
    for a, b, word in ((cp, bad_rv, b"rowval"), (bad_cp, rv, b"colptr")):
        a0, b0 = a.cpu().numpy().copy(), b.cpu().numpy().copy()
        with pytest.raises(fd.lib.FdError) as e:
            fd.matrix_colors_device(N, N, a, b)
        assert e.value.code == 2 and word in L.fd_last_error()
        with pytest.raises(fd.lib.FdError) as e:
            fd.check_colors_device(N, N, a, b, out)
        assert e.value.code == 2 and word in L.fd_last_error()
        assert _unchanged(a, a0) and _unchanged(b, b0)
    # NULL arguments and bad widths: FD_ERR_ARG
    nc = C.c_int64()
    args = lambda **kw: [kw.get("ctx", ctx.handle), N, N, kw.get("cp", cp.data_ptr()), kw.get("rv", rv.data_ptr()), kw.get("ib", 8), kw.get("base", 1),
                         kw.get("out", out.data_ptr()), kw.get("cb", 4), C.byref(nc)]
    for kw in (dict(ctx=None), dict(cp=None), dict(rv=None), dict(out=None), dict(ib=2), dict(cb=2), dict(cb=16), dict(base=2)):
        assert L.fd_color_columns_device(*args(**kw)) == 1, kw
        assert L.fd_color_check_device(*args(**kw)) == 1, kw
        assert L.fd_last_error()
    assert L.fd_color_check_device(*(args()[:-1] + [None])) == 1          # nowhere to put the count
    assert L.fd_color_columns_device(*(args()[:-1] + [None])) == 0        # ncolors_out is optional
    # the binding's own checks
    with pytest.raises(TypeError):
        fd.matrix_colors_device(N, N, cp, rv.to(torch.int32))
    with pytest.raises(TypeError):
        fd.matrix_colors_device(N, N, cp.cpu(), rv.cpu())
    # and after all of that the arrays are what they were, and the function still colours them
    assert _unchanged(cp, colptr) and _unchanged(rv, rowval)
    colors, n = fd.matrix_colors_device(N, N, cp, rv)
    assert fd.check_colors_device(N, N, cp, rv, colors) == 0 and 3 <= n <= 5
