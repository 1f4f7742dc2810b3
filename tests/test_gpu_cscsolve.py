"""The sparse consumer on the device (csrc/fdjac_cscsolve.hip): row lists, products and the BiCGStab solve BIT FOR BIT against the numpy
model (tests/csc_solve_model.py), the derived accuracy bound of tests/test_cscsolve_model_cpu.py on the device's own y, the failure
paths, and the path end to end behind a Jacobian the library has just stored."""
import os
import subprocess

import numpy as np
import pytest

import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P
import csc_solve_model as M
import test_cscsolve_model_cpu as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sp = H.sp                  # (SciPy: the reference of the accuracy bound)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, MAXIT = H.RTOL, H.MAXIT


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(got, want):
    return got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _solver(colptr, rowval, N, dtype=np.float64, idx=np.int64, base=0, device=False):
    cp, rv = (colptr + base).astype(idx), (rowval + base).astype(idx)
    if device:
        cp, rv = _dev(cp), _dev(rv)
    return fd.CscSolver((cp, rv, N), dtype=dtype, idx_base=base)


def _check_lists(s, rl):
    row_ptr, row_col, row_slot, diag, nlong = s.row_lists()
    assert np.array_equal(row_ptr.cpu().numpy(), rl.row_ptr)
    assert np.array_equal(row_col.cpu().numpy(), rl.row_col)
    assert np.array_equal(row_slot.cpu().numpy(), rl.row_slot)
    assert np.array_equal(diag.cpu().numpy(), rl.diag)
    assert nlong == rl.nlong


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("idx", [np.int32, np.int64])
def test_row_lists_equal_the_model(idx, base, device):
    for colptr, rowval, N in (M.lap5_pattern(37, 29), M.random_band_pattern(20000, 300, 6, 4)):
        _check_lists(_solver(colptr, rowval, N, idx=idx, base=base, device=device), M.RowLists(colptr, rowval, N))


def test_row_lists_with_empty_rows_empty_columns_and_a_dense_row():
    colptr, rowval, N = M.odd_pattern(4000, 77, 3000, 1)
    rl = M.RowLists(colptr, rowval, N)
    assert rl.nlong == 1 and (rl.lens == 0).any() and (np.diff(colptr) == 0).any()
    for device in (False, True):
        _check_lists(_solver(colptr, rowval, N, device=device), rl)


def test_a_bad_pattern_is_an_error_not_a_fault():
    colptr, rowval, N = M.tridiag_pattern(100)
    bad_row = rowval.copy(); bad_row[50] = 100
    unsorted = rowval.copy(); unsorted[[4, 5]] = unsorted[[5, 4]]
    bad_ptr = colptr.copy(); bad_ptr[10] = bad_ptr[12] + 1
    for cp, rv in ((colptr, bad_row), (colptr, unsorted), (bad_ptr, rowval)):
        for device in (False, True):
            with pytest.raises(fd.lib.FdError) as e:
                _solver(cp, rv, N, device=device)
            assert e.value.code == 2                   # FD_ERR_SHAPE


PRODUCT_PATTERNS = {
    "lap5": lambda: M.lap5_pattern(300, 200),
    "lap5_wide": lambda: M.lap5_pattern(2500, 40),              # reach 2500: beyond the LDS window's 1920
    "band": lambda: M.random_band_pattern(30000, 300, 6, 11),
    "tridiag": lambda: M.tridiag_pattern(20000),
    "odd": lambda: M.odd_pattern(4000, 77, 3000, 1),
}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(PRODUCT_PATTERNS))
def test_matvec_is_bit_identical_to_the_model(name, dtype, monkeypatch):
    colptr, rowval, N = PRODUCT_PATTERNS[name]()
    rl = M.RowLists(colptr, rowval, N)
    rng = np.random.default_rng(21)
    nz, v = rng.uniform(-1, 1, rowval.size).astype(dtype), rng.uniform(-1, 1, N).astype(dtype)
    Jd, vd = _dev(nz), _dev(v)
    solvers = [_solver(colptr, rowval, N, dtype=dtype)]
    monkeypatch.setenv("FDJAC_CSC_WINDOW", "0")             # no LDS window of v: the same bits
    solvers.append(_solver(colptr, rowval, N, dtype=dtype))
    for alpha, beta in ((0.0, 1.0), (1.0, -0.37), (-2.5, 0.75)):
        want = M.matvec(rl, alpha, beta, nz, v)
        want_t = M.matvec_t(rl, alpha, beta, nz, v)
        for s in solvers:
            for _ in range(2):
                y = torch.full((N,), float("nan"), dtype=Jd.dtype, device="cuda")
                s.matvec(Jd, vd, y, alpha, beta)
                assert _same_bits(y.cpu().numpy(), want), (name, alpha, beta)
                y.fill_(float("nan"))
                s.matvec(Jd, vd, y, alpha, beta, transpose=True)
                assert _same_bits(y.cpu().numpy(), want_t), (name, alpha, beta, "T")


def _device_solve(s, nz, b, gamma, rtol=RTOL, maxit=MAXIT, keep=False):
    s.set_options(rtol, maxit)
    s.set_policy(keep)
    y = torch.full((b.size,), 7.0, dtype=_dev(b).dtype, device="cuda")
    s.solve(_dev(nz), _dev(b), y, 1.0, -gamma)
    return y.cpu().numpy(), s.status()


@pytest.mark.parametrize("target", [0.5, 0.9, 0.99])
@pytest.mark.parametrize("name", ["lap5", "band", "tridiag"])
def test_solve_is_bit_identical_to_the_model_and_meets_the_derived_bound(name, target, monkeypatch):
    colptr, rowval, N, nz, b, gamma, J = H.make_case(name, target)
    rl = M.RowLists(colptr, rowval, N)
    want, wst = M.solve(rl, 1.0, -gamma, nz, b, RTOL, MAXIT)
    s = _solver(colptr, rowval, N)
    for _ in range(2):
        got, st = _device_solve(s, nz, b, gamma)
        print("%s %.2f: iterations %d (model %d) resid %.3e (model %.3e)" % (name, target, st["iterations"], wst["iterations"], st["resid"], wst["resid"]))
        assert st["flags"] == 0 and st["iterations"] == wst["iterations"]
        assert st["resid"] == wst["resid"] and st["bnorm"] == wst["bnorm"]
        assert _same_bits(got, want)
    monkeypatch.setenv("FDJAC_CSC_BATCH", "3")              # another batch size: not a bit, not the count
    got3, st3 = _device_solve(_solver(colptr, rowval, N), nz, b, gamma)
    assert st3 == st and _same_bits(got3, want)
    err, bound, delta = H.derived_bound_holds(J, gamma, b, got)
    print("    error %.3e bound %.3e delta %.3e" % (err, bound, delta))
    assert err <= bound


def test_solve_non_dominant_band_and_float32_are_bit_identical_to_the_model():
    colptr, rowval, N, nz, b, gamma, J = H.make_case("band", 3.0)
    rl = M.RowLists(colptr, rowval, N)
    want, wst = M.solve(rl, 1.0, -gamma, nz, b, RTOL, 500)
    got, st = _device_solve(_solver(colptr, rowval, N), nz, b, gamma, maxit=500)
    assert wst["flags"] == 0 and st["flags"] == 0 and st["iterations"] == wst["iterations"] and _same_bits(got, want)
    for name in ("lap5", "tridiag"):
        colptr, rowval, N, nz, b, gamma, J = H.make_case(name, 0.9, dtype=np.float32)
        rl = M.RowLists(colptr, rowval, N)
        want, wst = M.solve(rl, 1.0, -gamma, nz, b, 1e-6, MAXIT)
        got, st = _device_solve(_solver(colptr, rowval, N, dtype=np.float32), nz, b, gamma, rtol=1e-6)
        assert wst["flags"] == 0 and st["flags"] == 0 and st["iterations"] == wst["iterations"] and _same_bits(got, want)


@pytest.mark.parametrize("name", ["lap5", "tridiag"])
def test_failure_is_loud(name):
    colptr, rowval, N, nz, b, gamma, J = H.make_case(name, 3.0)
    rl = M.RowLists(colptr, rowval, N)
    s = _solver(colptr, rowval, N)
    want, wst = M.solve(rl, 1.0, -gamma, nz, b, RTOL, 500)
    got, st = _device_solve(s, nz, b, gamma, maxit=500)
    assert wst["flags"] in (1, 2) and st["flags"] == wst["flags"] and st["iterations"] == wst["iterations"] and np.all(np.isnan(got))
    wantk, _ = M.solve(rl, 1.0, -gamma, nz, b, RTOL, 500, keep_unconverged=True)
    gotk, stk = _device_solve(s, nz, b, gamma, maxit=500, keep=True)
    assert stk["flags"] == wst["flags"] and _same_bits(gotk, wantk) and np.all(np.isfinite(gotk))
    got1, st1 = _device_solve(s, nz, b, gamma, maxit=1)
    assert st1["flags"] == 1 and st1["iterations"] == 1 and np.all(np.isnan(got1))
    # the same solver is clean again on a dominant system
    colptr, rowval, N, nz, b, gamma, J = H.make_case(name, 0.5)
    got, st = _device_solve(s, nz, b, gamma)
    assert st["flags"] == 0 and np.all(np.isfinite(got))


def test_edge_cases_b_zero_zero_diagonal_and_n_one():
    colptr, rowval, N = M.tridiag_pattern(300)
    rl = M.RowLists(colptr, rowval, N)
    nz = np.random.default_rng(1).uniform(-1, 1, rowval.size)
    s = _solver(colptr, rowval, N)
    s.set_options(1e-10, 50)
    y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
    s.solve(_dev(nz), torch.zeros(N, dtype=torch.float64, device="cuda"), y, 1.0, -0.1)
    st = s.status()
    assert st == {"flags": 0, "iterations": 0, "resid": 0.0, "bnorm": 0.0} and bool((y == 0).all())
    nz0 = nz.copy(); nz0[rl.diag[17]] = 4.0
    s.solve(_dev(nz0), torch.ones(N, dtype=torch.float64, device="cuda"), y, 1.0, -0.25)
    st = s.status()
    assert st["flags"] == 2 and st["iterations"] == 0 and bool(torch.isnan(y).all())
    one = _solver(np.array([0, 1]), np.array([0]), 1)
    y1 = torch.zeros(1, dtype=torch.float64, device="cuda")
    one.solve(_dev(np.array([0.5])), _dev(np.array([3.0])), y1, 1.0, -0.5)
    assert one.status()["flags"] == 0 and one.status()["iterations"] == 1 and float(y1[0]) == 4.0


def test_implicit_step_on_a_five_point_jacobian_the_library_stored():
    nx, ny = 64, 50
    N = nx * ny
    colptr, rowval = P.lap5_csc(nx, ny)
    colors = P.lap5_colors(nx, ny)
    J = fd.SparseMatrixCSC(N, N, colptr, rowval, None)
    out = torch.zeros(rowval.size, dtype=torch.float64, device="cuda")
    x = _dev(np.random.default_rng(8).random(N) * 0.5)
    x0 = x.clone()
    plan = fd.make_plan(J, J, colors, "forward")
    f = fd.BuiltinF("lap5_nl", nx, ny)
    plan.set_lazy(f)
    plan.jacobian(f, x, [out])
    vals = out.cpu().numpy()
    A = sp.csc_matrix((vals, rowval - 1, colptr - 1), shape=(N, N))
    gamma = 0.9 / abs(A).sum(axis=1).max()
    b = np.random.default_rng(9).uniform(-1, 1, N)
    s = fd.CscSolver(J)
    s.set_options(RTOL, MAXIT)
    y = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    s.solve(out, _dev(b), y, 1.0, -gamma)
    st = s.status()
    assert st["flags"] == 0 and 1 <= st["iterations"] < MAXIT
    err, bound, delta = H.derived_bound_holds(A, float(gamma), b, y.cpu().numpy())
    print("end to end: iterations %d error %.3e bound %.3e delta %.3e" % (st["iterations"], err, bound, delta))
    assert err <= bound
    assert _same_bits(out.cpu().numpy(), vals) and bool((x == x0).all())


def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "csc_solve_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "csc_solve_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "status 0" in out.stdout, out.stdout
