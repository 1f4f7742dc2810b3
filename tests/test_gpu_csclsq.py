"""The least-squares consumer on the device (csrc/fdjac_csclsq.hip): the lists, both products and the preconditioned CGLS solve BIT FOR
BIT against the numpy model (tests/csc_lsq_model.py), the derived accuracy bound of tests/test_csclsq_model_cpu.py on the device's own
y, the failure paths, the path end to end behind a rectangular Jacobian the library has just stored, and the square solver beside it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as SM
import csc_lsq_model as LM
import test_csclsq_model_cpu as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, MAXIT = H.RTOL, H.MAXIT
_odd = {}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(got, want):
    return got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _lsq(colptr, rowval, M, N, dtype=np.float64, idx=np.int64, base=0, device=False):
    cp, rv = (colptr + base).astype(idx), (rowval + base).astype(idx)
    if device:
        cp, rv = _dev(cp), _dev(rv)
    return fd.CscLeastSquares((cp, rv, M, N), dtype=dtype, idx_base=base)


def odd_case():
    if not _odd:
        colptr, rowval, nz, M, N = LM.rect_odd()
        _odd["c"] = (colptr, rowval, nz, M, N, np.random.default_rng(2).uniform(-1, 1, M), LM.RectLists(colptr, rowval, M, N))
    return _odd["c"]


def _check_lists(s, rl):
    row_ptr, row_col, row_slot, nlong = s.row_lists()
    assert np.array_equal(row_ptr.cpu().numpy(), rl.row_ptr)
    assert np.array_equal(row_col.cpu().numpy(), rl.row_col)
    assert np.array_equal(row_slot.cpu().numpy(), rl.row_slot)
    assert nlong == rl.nlong
    assert np.array_equal(s.long_columns().cpu().numpy(), rl.long_cols)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("idx", [np.int32, np.int64])
def test_lists_equal_the_model(idx, base, device):
    for case in (H.band_case("big"), H.band_case("padded"), odd_case()):
        colptr, rowval, nz, M, N, b, rl = case
        _check_lists(_lsq(colptr, rowval, M, N, idx=idx, base=base, device=device), rl)


def shared_builder_case():
    """One SQUARE pattern for both consumers of the shared builder: N = 300 (two tiles of 256 rows), row 137 and column 201 of 40 entries
    (> 32: long), row 50 and column 60 empty, no diagonal entry in column 100.  The numpy models alone already agree on it (asserted)."""
    if "shared" not in _odd:
        N, long_row, long_col, empty_row, empty_col, no_diag = 300, 137, 201, 50, 60, 100
        entries = {(r, j) for j in range(N) for r in (j - 1, j, j + 2) if 0 <= r < N and r != long_row and j != long_col}
        entries |= {(long_row, 5 + 7 * k) for k in range(40)} | {(4 + 7 * k, long_col) for k in range(40)}      # (they share (137, 201))
        entries = sorted((j, r) for r, j in entries if r != empty_row and j != empty_col and (r, j) != (no_diag, no_diag))
        cols, rowval = np.array([e[0] for e in entries]), np.array([e[1] for e in entries], dtype=np.int64)
        colptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=N))]).astype(np.int64)
        sq, rect = SM.RowLists(colptr, rowval, N), LM.RectLists(colptr, rowval, N, N)
        for name in ("row_ptr", "row_col", "row_slot"):
            assert np.array_equal(getattr(sq, name), getattr(rect, name))
        assert sq.nlong == rect.nlong == 1 and sq.lens[long_row] == 40 and sq.lens[empty_row] == 0
        assert rect.long_cols.tolist() == [long_col] and rect.col_lens[long_col] == 40 and rect.col_lens[empty_col] == 0
        assert sq.diag[no_diag] == -1 and rect.col_lens[no_diag] > 0 and (sq.diag >= 0).sum() == N - 5      # (and 50, 60, 137, 201)
        _odd["shared"] = (colptr, rowval, N, sq, rect)
    return _odd["shared"]


@pytest.mark.parametrize("idx,base,device,dtype", [
    (np.int32, 0, False, np.float64), (np.int32, 0, True, np.float64), (np.int32, 1, False, np.float64), (np.int32, 1, True, np.float32),
    (np.int64, 0, False, np.float64), (np.int64, 0, True, np.float64), (np.int64, 1, False, np.float64), (np.int64, 1, True, np.float64)])
def test_both_consumers_get_the_same_lists_from_the_shared_builder(idx, base, device, dtype):
    colptr, rowval, N, sq, rect = shared_builder_case()
    cp, rv = (colptr + base).astype(idx), (rowval + base).astype(idx)
    if device:
        cp, rv = _dev(cp), _dev(rv)
    solver = fd.CscSolver((cp, rv, N), dtype=dtype, idx_base=base)
    lsq = fd.CscLeastSquares((cp, rv, N, N), dtype=dtype, idx_base=base)
    s_ptr, s_col, s_slot, s_diag, s_nlong = solver.row_lists()
    l_ptr, l_col, l_slot, l_nlong = lsq.row_lists()
    for got_s, got_l, name in ((s_ptr, l_ptr, "row_ptr"), (s_col, l_col, "row_col"), (s_slot, l_slot, "row_slot")):
        assert torch.equal(got_s, got_l), name
        assert np.array_equal(got_s.cpu().numpy(), getattr(sq, name)) and np.array_equal(got_l.cpu().numpy(), getattr(rect, name)), name
    assert np.array_equal(s_diag.cpu().numpy(), sq.diag) and int(s_diag[100]) == -1
    assert s_nlong == 1 and l_nlong == 1
    assert lsq.long_columns().cpu().numpy().tolist() == [201]
    rng = np.random.default_rng(33)
    nz, v = rng.uniform(-1, 1, rowval.size).astype(dtype), rng.uniform(-1, 1, N).astype(dtype)
    Jd, vd = _dev(nz), _dev(v)
    for transpose in (False, True):
        y = torch.full((N,), float("nan"), dtype=Jd.dtype, device="cuda")
        solver.matvec(Jd, vd, y, 0.5, -1.25, transpose=transpose)
        want = (SM.matvec_t if transpose else SM.matvec)(sq, 0.5, -1.25, nz, v)
        assert _same_bits(y.cpu().numpy(), want), ("solver", transpose)
        y = torch.full((N,), float("nan"), dtype=Jd.dtype, device="cuda")
        lsq.matvec(Jd, vd, y, transpose=transpose)
        assert _same_bits(y.cpu().numpy(), LM.matvec(rect, nz, v, transpose)), ("lsq", transpose)


def test_a_bad_pattern_is_an_error_not_a_fault():
    colptr, rowval, nz, M, N, b, rl = odd_case()
    assert M < N
    k = int(np.nonzero(np.diff(colptr) >= 2)[0][3])
    bad_row = rowval.copy(); bad_row[colptr[k + 1] - 1] = M              # a row that a square N x N pattern would allow
    unsorted = rowval.copy(); unsorted[[colptr[k], colptr[k] + 1]] = unsorted[[colptr[k] + 1, colptr[k]]]
    bad_ptr = colptr.copy(); bad_ptr[k] = bad_ptr[k + 1] + 1
    for cp, rv in ((colptr, bad_row), (colptr, unsorted), (bad_ptr, rowval)):
        for device in (False, True):
            with pytest.raises(fd.lib.FdError) as e:
                _lsq(cp, rv, M, N, device=device)
            assert e.value.code == 2                   # FD_ERR_SHAPE
    with pytest.raises(ValueError):                    # colptr against N + 1
        _lsq(colptr[:-1], rowval, M, N)
    with pytest.raises(ValueError):                    # the square solver keeps refusing a rectangular pattern
        fd.CscSolver(fd.SparseMatrixCSC(M, N, colptr + 1, rowval + 1, None))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["big", "padded", "odd"])
def test_products_are_bit_identical_to_the_model(name, dtype):
    colptr, rowval, nz, M, N, b, rl = odd_case() if name == "odd" else H.band_case(name)
    assert M % 256 and N % 256 and M % 1024 and N % 1024
    rng = np.random.default_rng(21)
    nz = nz.astype(dtype)
    s = _lsq(colptr, rowval, M, N, dtype=dtype)
    Jd = _dev(nz)
    for transpose, n_in, n_out in ((False, N, M), (True, M, N)):
        v = rng.uniform(-1, 1, n_in).astype(dtype)
        want = LM.matvec(rl, nz, v, transpose)
        vd = _dev(v)
        for _ in range(2):
            y = torch.full((n_out,), float("nan"), dtype=Jd.dtype, device="cuda")
            s.matvec(Jd, vd, y, transpose=transpose)
            assert _same_bits(y.cpu().numpy(), want), (name, transpose)


def _device_solve(s, nz, b, mu, kind, rtol=RTOL, maxit=MAXIT, keep=False, N=None):
    s.set_options(rtol, maxit)
    s.set_policy(keep)
    bd = _dev(b)
    y = torch.full((s.N,), 7.0, dtype=bd.dtype, device="cuda")
    r = torch.full((s.M,), 7.0, dtype=bd.dtype, device="cuda")
    s.solve(_dev(nz), bd, y, mu, kind, r_out=r)
    return y.cpu().numpy(), r.cpu().numpy(), s.status()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mu,kind", LM.MU_W)
@pytest.mark.parametrize("name", ["big", "padded"])
def test_solve_is_bit_identical_to_the_model_and_meets_the_derived_bound(name, mu, kind, dtype):
    colptr, rowval, nz, M, N, b, rl = H.band_case(name, dtype)
    want_y, want_r, wst = H.model_solution(name, mu, kind, dtype)
    assert wst["flags"] == 0
    s = _lsq(colptr, rowval, M, N, dtype=dtype)
    for _ in range(2):                                   # twice on one consumer: the ticket and the `done` word are reused
        y, r, st = _device_solve(s, nz, b, mu, kind)
        print("%s mu %g kind %d: iterations %d (model %d) grad %.3e (model %.3e)" % (name, mu, kind, st["iterations"], wst["iterations"], st["grad"], wst["grad"]))
        assert st == wst
        assert _same_bits(y, want_y) and _same_bits(r, want_r)
    if dtype == np.float64:
        err, bound, rel = H.derived_bound(name, mu, kind, y)
        print("    error %.3e bound %.3e = %.3e ||y_ref||" % (err, bound, rel))
        assert rel <= 1e-6
        assert err <= bound
    # without r_out
    y2 = torch.full((N,), 7.0, dtype=_dev(b).dtype, device="cuda")
    s.solve(_dev(nz), _dev(b), y2, mu, kind)
    assert _same_bits(y2.cpu().numpy(), want_y) and s.status() == wst


def test_solve_is_bit_identical_under_batch_sizes_1_and_8():
    """Both band cases, the four (mu, W) pairs, FDJAC_CSC_BATCH in {1, 8}: in a child process of its own
    (tests/csclsq_switch_child.py) with FDJAC_TEST_SWITCHES=1."""
    env = dict(os.environ, FDJAC_TEST_SWITCHES="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "csclsq_switch_child.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout and out.stdout.count(": ok ") == 16 and "MISMATCH" not in out.stdout


def test_failure_paths_are_loud_and_equal_the_model():
    colptr, rowval, nz, M, N, b, rl = odd_case()
    s = _lsq(colptr, rowval, M, N)
    # the iterations run out
    wy, wr, wst = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nz, b, RTOL, 3)
    y, r, st = _device_solve(s, nz, b, 0.5, LM.DAMP_IDENTITY, maxit=3)
    assert wst["flags"] == 1 and st == wst and st["iterations"] == 3 and np.all(np.isnan(y)) and np.all(np.isnan(r))
    wy, wr, wst = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nz, b, RTOL, 3, keep_unconverged=True)
    y, r, st = _device_solve(s, nz, b, 0.5, LM.DAMP_IDENTITY, maxit=3, keep=True)
    assert st == wst and st["flags"] == 1 and _same_bits(y, wy) and _same_bits(r, wr) and np.all(np.isfinite(y))
    # breakdown: the empty column that nothing damps (mu = 0; W = diag(g))
    for mu, kind in ((0.0, LM.DAMP_IDENTITY), (0.5, LM.DAMP_COLNORM)):
        wy, wr, wst = LM.solve(rl, mu, kind, nz, b, RTOL, MAXIT)
        y, r, st = _device_solve(s, nz, b, mu, kind)
        assert wst["flags"] == 2 and st == wst and st["iterations"] == 0 and np.all(np.isnan(y)) and np.all(np.isnan(r))
    wy, wr, wst = LM.solve(rl, 0.0, LM.DAMP_IDENTITY, nz, b, RTOL, MAXIT, keep_unconverged=True)
    y, r, st = _device_solve(s, nz, b, 0.0, LM.DAMP_IDENTITY, keep=True)
    assert st == wst and st["flags"] == 2 and _same_bits(y, wy) and _same_bits(r, wr)
    # the same consumer is clean again: Levenberg's damping reaches the empty columns
    wy, wr, wst = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, nz, b, RTOL, MAXIT)
    y, r, st = _device_solve(s, nz, b, 0.5, LM.DAMP_IDENTITY)
    assert wst["flags"] == 0 and st == wst and _same_bits(y, wy) and _same_bits(r, wr)
    # b supported on the empty rows: J^T b = 0 bit for bit, no iteration
    b0 = np.where(rl.lens == 0, b, 0.0)
    y, r, st = _device_solve(s, nz, b0, 0.5, LM.DAMP_IDENTITY)
    assert st == {"flags": 0, "iterations": 0, "grad": 0.0, "grad0": 0.0} and not y.any() and _same_bits(r, b0)
    # arguments
    yd, bd, nzd = torch.zeros(N, dtype=torch.float64, device="cuda"), _dev(b), _dev(nz)
    for mu, kind in ((0.5, 2), (0.5, -1), (-1e-3, 0), (float("nan"), 1)):
        with pytest.raises(fd.lib.FdError) as e:
            s.solve(nzd, bd, yd, mu, kind)
        assert e.value.code == 1                       # FD_ERR_ARG


def test_gauss_newton_step_on_a_rectangular_jacobian_the_library_stored():
    n = 2500                                             # f: R^2n -> R^n, J = [diag(2 (x1 - 3) + x2), diag(x1 + 2 (x2 + 4))]
    M, N = n, 2 * n
    colptr, rowval = np.arange(N + 1, dtype=np.int64) + 1, (np.arange(N, dtype=np.int64) % n) + 1
    colorvec = np.concatenate([np.full(n, 1), np.full(n, 2)])
    rng = np.random.default_rng(8)
    x0 = rng.uniform(0.5, 2.5, N)
    J = fd.SparseMatrixCSC(M, N, colptr, rowval, _dev(np.zeros(N)))
    cache = fd.JacobianCache(_dev(x0.copy()), _dev(np.zeros(M)), _dev(np.zeros(M)), "forward", sparsity=J, colorvec=colorvec)
    f = fd.BuiltinF("nonsquare", n)
    fd.finite_difference_jacobian_b(J, f, _dev(x0), cache)
    b = rng.uniform(-1, 1, M)
    s = fd.CscLeastSquares(J)
    y = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    r = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
    s.solve(J, _dev(b), y, 0.5, "identity", r_out=r)     # the stored nzval goes straight in
    st = s.status()
    vals = J.nzval.cpu().numpy()
    x1, x2 = x0[:n], x0[n:]
    exact = np.concatenate([2 * (x1 - 3) + x2, x1 + 2 * (x2 + 4)])
    assert np.linalg.norm(vals - exact) <= 1e-6 * np.linalg.norm(exact)
    rl = LM.RectLists(colptr - 1, rowval - 1, M, N)
    wy, wr, wst = LM.solve(rl, 0.5, LM.DAMP_IDENTITY, vals, b)
    print("end to end: iterations %d grad %.3e grad0 %.3e" % (st["iterations"], st["grad"], st["grad0"]))
    assert wst["flags"] == 0 and st == wst and st["iterations"] >= 1
    assert _same_bits(y.cpu().numpy(), wy) and _same_bits(r.cpu().numpy(), wr)


def test_the_square_solver_is_untouched_by_a_least_squares_solve_beside_it():
    colptr, rowval, N = SM.tridiag_pattern(5000)
    rng = np.random.default_rng(5)
    nz, b = rng.uniform(-1, 1, rowval.size), rng.uniform(-1, 1, N)
    sq = fd.CscSolver((colptr, rowval, N), idx_base=0)
    sq.set_options(1e-12, 60)

    def square():
        y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        sq.solve(_dev(nz), _dev(b), y, 1.0, -0.2)
        return y.cpu().numpy(), sq.status()

    before, st_before = square()
    want, wst = SM.solve(SM.RowLists(colptr, rowval, N), 1.0, -0.2, nz, b, 1e-12, 60)
    assert st_before == wst and st_before["flags"] == 0 and _same_bits(before, want)
    lc, lr, lnz, LMm, LN, lb, lrl = H.band_case("padded")
    ls = _lsq(lc, lr, LMm, LN)
    assert ls.ctx is sq.ctx
    _, _, lst = _device_solve(ls, lnz, lb, 1e-2, LM.DAMP_IDENTITY)
    assert lst["flags"] == 0
    after, st_after = square()
    assert st_after == st_before and _same_bits(after, before)


def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "csc_lsq_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "csc_lsq_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "status 0" in out.stdout, out.stdout
