"""The products of the three consumers on SparseMatrixCSC storage at the edges of the code they share (csrc/fdjac_csc_common.h: the
gathered sum in groups of eight, the split at 32 entries, the strided sum of a long line, the tile of 256 lines), BIT FOR BIT against the
numpy models.  The STAIRCASE, N = 600: row r holds L(r) entries at the columns (3 r + 13 k) mod 600, k < L(r) (distinct: 13 and 600 are
coprime), L(r) = r mod 41 except L(570) = 257, L(580) = 600, L(590) = 513.  So every length 0 .. 40 occurs (an empty line, 1, 7 / 8 / 9,
15 / 16 / 17, 31 / 32 / 33), 114 rows are long, the long rows take one, two (257: a full pass and one entry) and three passes, and `order`
has two full tiles and a partial one.  Its transpose puts the same lengths on the columns (the long-column kernel and the column tile of
the least-squares consumer)."""
import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_lsq_model as LM
import csc_solve_model as SM
import csc_tr_model as TM

N = 600
LONG_EXCEPTIONS = {570: 257, 580: 600, 590: 513}
SHORT_LINE, LONG_LINE = 9, 570              # the lines of the signed-zero case


def line_lengths():
    L = np.arange(N) % 41
    for r, n in LONG_EXCEPTIONS.items():
        L[r] = n
    return L


def staircase(transposed=False):
    """(colptr, rowval, N) of the staircase, or of its transpose."""
    L = line_lengths()
    rows = np.repeat(np.arange(N), L)
    k = np.concatenate([np.arange(n) for n in L])
    cols = (3 * rows + 13 * k) % N
    if transposed:
        rows, cols = cols, rows
    order = np.lexsort((rows, cols))         # by column, within a column by row
    colptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=N))]).astype(np.int64)
    return colptr, rows[order].astype(np.int64), N


def test_the_staircase_has_every_length_at_the_edges():
    L = line_lengths()
    colptr, rowval, n = staircase()
    rl = SM.RowLists(colptr, rowval, n)
    assert rowval.size == 13116 and np.array_equal(rl.lens, L)
    assert all(np.all(np.diff(rl.row_col[rl.row_ptr[r]:rl.row_ptr[r + 1]]) > 0) for r in range(N))      # distinct, ascending
    assert set(L.tolist()) == set(range(41)) | {257, 513, 600}
    assert rl.nlong == 114 and int((L > SM.LONG).sum()) == 114
    assert (N + SM.BLOCK - 1) // SM.BLOCK == 3 and N % SM.BLOCK == 88
    tcolptr, trowval, _ = staircase(transposed=True)
    assert trowval.size == 13116 and np.array_equal(np.diff(tcolptr), L)
    rect = LM.RectLists(tcolptr, trowval, N, N)
    assert np.array_equal(rect.col_lens, L) and rect.long_cols.size == 114
    rng = np.random.default_rng(1)
    for dtype in (np.float64, np.float32):
        nz, v = rng.uniform(-1, 1, rowval.size).astype(dtype), rng.uniform(-1, 1, N).astype(dtype)
        assert np.isfinite(SM.matvec(rl, 1.0, -0.37, nz, v)).all() and np.isfinite(SM.matvec_t(rl, 1.0, -0.37, nz, v)).all()
        assert np.isfinite(LM.matvec(rect, nz, v)).all() and np.isfinite(LM.matvec(rect, nz, v, True)).all()


try:                       # (the test above needs no torch)
    import torch
except ImportError:
    torch = None
PATTERNS = [False, True]
IDS = ["staircase", "transpose"]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    u = np.uint64 if want.dtype == np.float64 else np.uint32
    return got.dtype == want.dtype and np.array_equal(got.view(u), want.view(u))


def _twice(call, n_out, torch_dtype, want, what):
    """Every product twice into a NaN-filled y."""
    for _ in range(2):
        y = torch.full((n_out,), float("nan"), dtype=torch_dtype, device="cuda")
        call(y)
        assert _same_bits(y.cpu().numpy(), want), what


def _values(dtype, seed, size):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, size).astype(dtype), rng.uniform(-1, 1, N).astype(dtype)


def _check_solver(colptr, rowval, nz, v, monkeypatch, what):
    rl = SM.RowLists(colptr, rowval, N)
    Jd, vd = _dev(nz), _dev(v)
    solvers = [fd.CscSolver((colptr, rowval, N), dtype=nz.dtype, idx_base=0)]
    monkeypatch.setenv("FDJAC_CSC_WINDOW", "0")             # no LDS window of v: the same bits
    solvers.append(fd.CscSolver((colptr, rowval, N), dtype=nz.dtype, idx_base=0))
    monkeypatch.delenv("FDJAC_CSC_WINDOW")
    for alpha, beta in ((0.0, 1.0), (1.0, -0.37)):
        want, want_t = SM.matvec(rl, alpha, beta, nz, v), SM.matvec_t(rl, alpha, beta, nz, v)
        for w, s in enumerate(solvers):
            _twice(lambda y: s.matvec(Jd, vd, y, alpha, beta), N, Jd.dtype, want, (what, "solver", alpha, beta, w))
            _twice(lambda y: s.matvec(Jd, vd, y, alpha, beta, transpose=True), N, Jd.dtype, want_t, (what, "solver T", alpha, beta, w))


def _check_lsq(colptr, rowval, nz, v, what):
    rect = LM.RectLists(colptr, rowval, N, N)
    Jd, vd = _dev(nz), _dev(v)
    s = fd.CscLeastSquares((colptr, rowval, N, N), dtype=nz.dtype, idx_base=0)
    for transpose in (False, True):
        _twice(lambda y: s.matvec(Jd, vd, y, transpose=transpose), N, Jd.dtype, LM.matvec(rect, nz, v, transpose), (what, "lsq", transpose))


def _check_tr(colptr, rowval, nz, v, what):
    rl = TM.RowLists(colptr, rowval, N)
    Hd, vd = _dev(nz), _dev(v)
    s = fd.CscTrustRegion((colptr, rowval, N), idx_base=0)
    for lam in (0.0, 0.5):
        _twice(lambda y: s.matvec(Hd, vd, y, lam), N, torch.float64, TM.matvec(rl, lam, nz, v), (what, "tr", lam))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("transposed", PATTERNS, ids=IDS)
def test_solver_products_are_bit_identical_to_the_model(transposed, dtype, monkeypatch):
    colptr, rowval, _ = staircase(transposed)
    nz, v = _values(dtype, 31, rowval.size)
    _check_solver(colptr, rowval, nz, v, monkeypatch, (transposed, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("transposed", PATTERNS, ids=IDS)
def test_least_squares_products_are_bit_identical_to_the_model(transposed, dtype):
    colptr, rowval, _ = staircase(transposed)
    nz, v = _values(dtype, 32, rowval.size)
    _check_lsq(colptr, rowval, nz, v, (transposed, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("transposed", PATTERNS, ids=IDS)
def test_trust_region_products_are_bit_identical_to_the_model(transposed):
    colptr, rowval, _ = staircase(transposed)      # (the product does not require symmetry)
    nz, v = _values(np.float64, 33, rowval.size)
    _check_tr(colptr, rowval, nz, v, transposed)


@pytest.mark.gpu
@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["+0", "-0"])
def test_lines_of_signed_zeros_sum_to_plus_zero_on_all_three_consumers(zero, monkeypatch):
    """One short and one long line hold only `zero` and meet only negative v: every product is a zero of either sign, added to a +0.0
    accumulator, so the line's sum is +0.0 -- and y there is whatever the consumer's own epilogue makes of it (alpha v_r + beta 0,
    0 + lambda v_r, or the plain +0.0; an epilogue borrowed from another consumer, 0 v_r + t, would differ in the sign of a zero)."""
    for transposed in PATTERNS:
        colptr, rowval, _ = staircase(transposed)
        nz, v = _values(np.float64, 34, rowval.size)
        if transposed:      # the lines are columns: storage order
            slots = np.concatenate([np.arange(colptr[j], colptr[j + 1]) for j in (SHORT_LINE, LONG_LINE)])
            v[rowval[slots]] = -np.abs(v[rowval[slots]])
        else:
            rl = SM.RowLists(colptr, rowval, N)
            at = np.concatenate([np.arange(rl.row_ptr[r], rl.row_ptr[r + 1]) for r in (SHORT_LINE, LONG_LINE)])
            slots = rl.row_slot[at]
            v[rl.row_col[at]] = -np.abs(v[rl.row_col[at]])
        assert slots.size == SHORT_LINE + LONG_EXCEPTIONS[LONG_LINE]
        nz[slots] = zero
        assert np.all(np.signbit(nz[slots]) == np.signbit(zero))
        rect = LM.RectLists(colptr, rowval, N, N)
        got = LM.matvec(rect, nz, v, transposed)[[SHORT_LINE, LONG_LINE]]
        assert np.all(got == 0.0) and not np.signbit(got).any()
        _check_solver(colptr, rowval, nz, v, monkeypatch, (transposed, zero))
        _check_lsq(colptr, rowval, nz, v, (transposed, zero))
        _check_tr(colptr, rowval, nz, v, (transposed, zero))
