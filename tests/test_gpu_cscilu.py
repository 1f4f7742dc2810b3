"""The block ILU(0) preconditioner of the sparse consumer on the device (csrc/fdjac_cscsolve.hip: k_cs_ilu_factor, k_cs_ilu_apply): the
levels, the factors, y, the iteration count, the residual norm and the flags BIT FOR BIT against the numpy model
(tests/csc_ilu_model.py); the switches between the preconditioners; the failure paths; and the path end to end behind a Jacobian the
library has just stored."""
import os
import subprocess
import sys

import numpy as np
import pytest

import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P
import csc_solve_model as M
import csc_block_model as BM
import csc_ilu_model as IM
import test_cscilu_model_cpu as H
import test_cscsolve_model_cpu as HJ

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, MAXIT = H.RTOL, H.MAXIT


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _solver(colptr, rowval, N, dtype=np.float64, idx=np.int64, base=0, device=False):
    cp, rv = (colptr + base).astype(idx), (rowval + base).astype(idx)
    if device:
        cp, rv = _dev(cp), _dev(rv)
    return fd.CscSolver((cp, rv, N), dtype=dtype, idx_base=base)


def _device_solve(s, nz, b, alpha, beta, rtol=RTOL, maxit=MAXIT, keep=False):
    s.set_options(rtol, maxit)
    s.set_policy(keep)
    y = torch.full((b.size,), 7.0, dtype=_dev(b).dtype, device="cuda")
    s.solve(_dev(nz), _dev(b), y, alpha, beta)
    return y.cpu().numpy(), s.status()


def _far_pattern():
    """N = 2048, entries at (i, i) and (i, i +- 1024): with bs = 1024 a block's rows all sit on level 0."""
    n = 2048
    rows = [[r for r in (c - 1024, c, c + 1024) if 0 <= r < n] for c in range(n)]
    colptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return colptr, np.array([r for rs in rows for r in rs], dtype=np.int64), n


# ---- 1. levels and factors ----------------------------------------------------------------------------------------------------------------
FACTOR_CASES = [("tridiag100", lambda: M.tridiag_pattern(100), (2, 7, 64, 100, 1024)),
                ("lap5_12x9", lambda: M.lap5_pattern(12, 9), (5, 36, 64, 108)),
                ("ragged300", lambda: H.ragged_pattern(), (64, 256)),
                ("dense8x4", lambda: BM.block_tridiag_pattern(4, 8), (8, 16)),
                ("n1", lambda: (np.array([0, 1]), np.array([0]), 1), (2,)),
                ("bs_plus_1", lambda: M.tridiag_pattern(65), (64,)),
                ("far2048", _far_pattern, (1024,))]


@pytest.mark.parametrize("case", FACTOR_CASES, ids=lambda c: c[0])
def test_levels_and_factors_equal_the_model_bit_for_bit(case):
    name, pat, sizes = case
    colptr, rowval, N = pat()
    rl = M.RowLists(colptr, rowval, N)
    nz = H.values_for(rowval, 12)
    b = np.random.default_rng(2).standard_normal(N)
    alpha, beta = 1.0, -0.1
    for bs in sizes:
        sch = IM.Schedule(rl, bs)
        if name == "far2048":
            assert sch.lev_f.max() == 0 and sch.lev_b.max() == 0
        for dtype in (np.float64, np.float32):
            nzt, bt = nz.astype(dtype), b.astype(dtype)
            lu, u, bad = IM.factor(sch, alpha, beta, nzt)
            assert not bad
            for device in (False, True):
                for idx in (np.int32, np.int64):
                    for base in (0, 1):
                        s = _solver(colptr, rowval, N, dtype=dtype, idx=idx, base=base, device=device)
                        s.set_block_ilu(bs)
                        lev_f, lev_b, max_f, max_b = s.ilu_levels()
                        what = (name, bs, dtype, device, idx, base)
                        assert np.array_equal(lev_f.cpu().numpy(), sch.lev_f) and np.array_equal(lev_b.cpu().numpy(), sch.lev_b), what
                        assert max_f == int(sch.lev_f.max()) and max_b == int(sch.lev_b.max()), what
                        _device_solve(s, nzt, bt, alpha, beta, maxit=1)
                        glu, gu, gbs = s.ilu_factors()
                        assert gbs == bs and _same_bits(glu.cpu().numpy(), lu) and _same_bits(gu.cpu().numpy(), u), what


# ---- 2. the solve ------------------------------------------------------------------------------------------------------------------------
def test_solve_is_bit_identical_to_the_model_under_every_batch_and_window_switch():
    """The 5-point 12 x 9 case (bs 36, 64) and the ragged case (bs 64, 256; a row of more than 32 entries: the long-row launches run
    beside the PC = 1 kernels), FDJAC_CSC_BATCH in {1, 8} x FDJAC_CSC_WINDOW in {0, 1}: in a child process of its own
    (tests/cscilu_switch_child.py) with FDJAC_TEST_SWITCHES=1."""
    env = dict(os.environ, FDJAC_TEST_SWITCHES="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cscilu_switch_child.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout and out.stdout.count(": ok ") == 16 and "MISMATCH" not in out.stdout


def test_float32_solve_is_bit_identical_to_the_model():
    colptr, rowval, N, nz, b, gamma = H.grid_case("convdiff_g50", 12, 9)
    nz32, b32 = nz.astype(np.float32), b.astype(np.float32)
    want, wst = IM.solve(M.RowLists(colptr, rowval, N), 1.0, -gamma, nz32, b32, 1e-6, MAXIT, bs=36)
    s = _solver(colptr, rowval, N, dtype=np.float32)
    s.set_block_ilu(36)
    got, st = _device_solve(s, nz32, b32, 1.0, -gamma, rtol=1e-6)
    assert wst["flags"] == 0 and wst["iterations"] >= 2 and st == wst and _same_bits(got, want)


# ---- 3. breakdowns -----------------------------------------------------------------------------------------------------------------------
def test_a_bad_pivot_is_a_breakdown_not_a_fault():
    for name, colptr, rowval, N, alpha, beta, nz, b, bs in H.breakdown_cases():
        s = _solver(colptr, rowval, N)
        s.set_block_ilu(bs)
        got, st = _device_solve(s, nz, b, alpha, beta)
        assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(got)), name
        kept, stk = _device_solve(s, nz, b, alpha, beta, keep=True)
        assert stk["flags"] == 2 and stk["iterations"] == 0 and np.array_equal(kept, np.zeros(N)), name
        # the same solver is clean again on regular values
        good = H.values_for(rowval, 12)
        want, wst = IM.solve(M.RowLists(colptr, rowval, N), 1.0, -0.1, good, b, RTOL, MAXIT, bs=bs)
        got, st = _device_solve(s, good, b, 1.0, -0.1)
        assert st == wst and st["flags"] == 0 and _same_bits(got, want), name


# ---- 4. switching ------------------------------------------------------------------------------------------------------------------------
def test_switching_between_the_preconditioners_leaves_nothing_behind():
    colptr, rowval, N, nz, b, gamma = H.grid_case("lap5_g10", 24, 20)
    rl = M.RowLists(colptr, rowval, N)
    args = (nz, b, 1.0, -gamma)
    fresh_j, fst_j = _device_solve(_solver(colptr, rowval, N), *args)
    fb = _solver(colptr, rowval, N)
    fb.set_preconditioner("block_jacobi", 8)
    fresh_b, fst_b = _device_solve(fb, *args)
    s = _solver(colptr, rowval, N)
    s.set_block_ilu(64)
    one, st1 = _device_solve(s, *args)
    two, st2 = _device_solve(s, *args)
    want, wst = IM.solve(rl, 1.0, -gamma, nz, b, RTOL, MAXIT, bs=64)
    assert st1 == wst and st1["flags"] == 0 and _same_bits(one, want) and st2 == st1 and _same_bits(two, one)
    assert not _same_bits(one, fresh_j) and st1["iterations"] < fst_j["iterations"]
    s.set_preconditioner("jacobi")
    again, ast = _device_solve(s, *args)
    assert ast == fst_j and _same_bits(again, fresh_j)
    s.set_block_ilu(64)
    s.set_preconditioner("block_jacobi", 8)
    again, ast = _device_solve(s, *args)
    assert ast == fst_b and _same_bits(again, fresh_b)
    s.set_block_ilu(100)                                             # another size on the same solver: the schedule is rebuilt
    other, ost = _device_solve(s, *args)
    f100 = _solver(colptr, rowval, N)
    f100.set_block_ilu(100)
    fresh100, fst100 = _device_solve(f100, *args)
    want100, wst100 = IM.solve(rl, 1.0, -gamma, nz, b, RTOL, MAXIT, bs=100)
    assert ost == fst100 == wst100 and _same_bits(other, fresh100) and _same_bits(other, want100) and s.ilu_factors()[2] == 100


# ---- 5. bad arguments --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_errors():
    colptr, rowval, N = M.tridiag_pattern(100)
    s = _solver(colptr, rowval, N)
    for size in (1, 0, -1, 1025):
        assert s.Lt.fd_csc_solver_set_block_ilu(s.handle, size) == 1, size            # FD_ERR_ARG
    assert s.Lt.fd_csc_solver_set_block_ilu(None, 64) == 1
    assert s.Lt.fd_csc_solver_ilu_levels(None, None, None, None, None) == 1
    assert s.Lt.fd_csc_solver_ilu_factors(None, None, None, None, None) == 1
    assert s.Lt.fd_csc_solver_set_preconditioner(s.handle, 2, 8) == 1                 # no third kind
    with pytest.raises(fd.lib.FdError) as e:
        s.ilu_levels()                                                                # block ILU is not set
    assert e.value.code == 3
    s.set_block_ilu(64)
    with pytest.raises(fd.lib.FdError) as e:
        s.ilu_factors()                                                               # no block-ILU solve yet
    assert e.value.code == 3
    assert s.ilu_levels()[2] == 63
    s.set_block_ilu(32)                                                               # a new schedule: its factors do not exist yet either
    with pytest.raises(fd.lib.FdError) as e:
        s.ilu_factors()
    assert e.value.code == 3


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------------
def test_implicit_euler_step_on_a_five_point_jacobian_the_library_stored():
    sp = HJ.sp
    nx, ny = 40, 30
    N = nx * ny
    colptr, rowval = P.lap5_csc(nx, ny)
    J = fd.SparseMatrixCSC(N, N, colptr, rowval, None)
    out = torch.zeros(rowval.size, dtype=torch.float64, device="cuda")
    xh = np.random.default_rng(8).random(N) * 0.5
    x = _dev(xh)
    plan = fd.make_plan(J, J, P.lap5_colors(nx, ny), "forward")
    f = fd.BuiltinF("lap5_nl", nx, ny)
    plan.set_lazy(f)
    plan.jacobian(f, x, [out])
    vals = out.cpu().numpy()
    A = sp.csc_matrix((vals, rowval - 1, colptr - 1), shape=(N, N))
    # one implicit-Euler step x1 = x + y of x' = f(x) with h = 1: (I - h J(x)) y = h f(x); f = the 5-point sum - 4 x + x^2 x_east on the host
    h = 1.0
    g = xh.reshape(ny, nx)
    pad = np.pad(g, 1)
    e = pad[1:-1, 2:]
    fx = ((((pad[1:-1, :-2] + e) + pad[:-2, 1:-1]) + pad[2:, 1:-1]) - 4.0 * g) + (g * g) * e
    b = (h * fx).reshape(-1)
    s = fd.CscSolver(J)
    s.set_options(HJ.RTOL, MAXIT)
    res = {}
    for kind in ("jacobi", "ilu"):
        if kind == "ilu":
            s.set_block_ilu(256)
        y = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        s.solve(out, _dev(b), y, 1.0, -h)                            # nzval never left the device
        st = s.status()
        err, bound, delta = HJ.derived_bound_holds(A, h, b, y.cpu().numpy())
        print("end to end, %s: iterations %d error %.3e bound %.3e delta %.3e" % (kind, st["iterations"], err, bound, delta))
        assert st["flags"] == 0 and 1 <= st["iterations"] < MAXIT
        assert err <= bound
        res[kind] = st["iterations"]
    assert res["ilu"] < res["jacobi"]
    assert _same_bits(out.cpu().numpy(), vals)


# ---- 7. the C client ---------------------------------------------------------------------------------------------------------------------
def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "csc_ilu_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "csc_ilu_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "csc ilu: PASS" in out.stdout, out.stdout
