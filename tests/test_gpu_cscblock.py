"""The block-Jacobi preconditioner of the sparse consumer on the device (csrc/fdjac_cscsolve.hip: k_cs_binv, k_cs_bapply): the inverses,
y, the iteration count, the residual norm and the flags BIT FOR BIT against the numpy model (tests/csc_block_model.py); the switch
back to the diagonal; the failure paths; and the path end to end behind a Jacobian the library has just stored."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as M
import csc_block_model as BM
import test_cscblock_model_cpu as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, MAXIT, GAMMA = H.RTOL, H.MAXIT, H.GAMMA


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


def _device_solve(s, nz, b, gamma=GAMMA, rtol=RTOL, maxit=MAXIT, keep=False):
    s.set_options(rtol, maxit)
    s.set_policy(keep)
    y = torch.full((b.size,), 7.0, dtype=_dev(b).dtype, device="cuda")
    s.solve(_dev(nz), _dev(b), y, 1.0, -gamma)
    return y.cpu().numpy(), s.status()


# ---- 5. the inverses ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [2, 3, 5, 8, 16, 31, 32])
def test_block_inverses_equal_the_model_bit_for_bit(bs):
    # N = 24 bs (one block per cell) and N = 1001 = 7 * 11 * 13 (no multiple of any of the sizes: the blocks cut across the cells)
    for colptr, rowval, nz, N in (BM.reaction_diffusion(6, 4, bs, 1e3, 1e3, 0.3, bs), BM.reaction_diffusion(11, 13, 7, 1e2, 1e2, 0.3, bs)):
        assert (N % bs == 0) == (N == 24 * bs)
        b = np.random.default_rng(2).standard_normal(N)
        for dtype in (np.float64, np.float32):
            nzt, bt = nz.astype(dtype), b.astype(dtype)
            want, bad = BM.block_inverses(colptr, rowval, N, 1.0, -GAMMA, nzt, bs)
            assert not bad
            for device in (False, True):
                for idx in (np.int32, np.int64):
                    for base in (0, 1):
                        s = _solver(colptr, rowval, N, dtype=dtype, idx=idx, base=base, device=device)
                        s.set_preconditioner("block_jacobi", bs)
                        _device_solve(s, nzt, bt, maxit=1)
                        got = s.block_inverses().cpu().numpy()
                        assert _same_bits(got, want), (bs, N, dtype, device, idx, base)


def test_bad_arguments_are_errors():
    colptr, rowval, N = M.tridiag_pattern(100)
    s = _solver(colptr, rowval, N)
    for kind, size in ((2, 8), (-1, 8), (1, 1), (1, 33), (1, 0)):
        rc = s.Lt.fd_csc_solver_set_preconditioner(s.handle, kind, size)
        assert rc == 1, (kind, size)                                 # FD_ERR_ARG
    with pytest.raises(fd.lib.FdError) as e:
        s.block_inverses()                                           # no block-Jacobi solve yet
    assert e.value.code == 3
    with pytest.raises(ValueError):
        s.set_preconditioner("ilu")
    s.set_preconditioner("jacobi", 77)                               # the size is ignored for kind 0


# ---- 6. the solve ------------------------------------------------------------------------------------------------------------------------
def test_solve_is_bit_identical_to_the_model_under_every_batch_and_window_switch():
    """Every row of the table and the block-tridiagonal 32 x 32 pattern, FDJAC_CSC_BATCH in {1, 8} x FDJAC_CSC_WINDOW in {0, 1}: in a
    child process of its own (tests/cscblock_switch_child.py) with FDJAC_TEST_SWITCHES=1."""
    env = dict(os.environ, FDJAC_TEST_SWITCHES="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cscblock_switch_child.py")], capture_output=True, text=True, env=env, timeout=900)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout and out.stdout.count(": ok ") == 40 and "MISMATCH" not in out.stdout


def test_float32_solve_is_bit_identical_to_the_model():
    colptr, rowval, nz, N, b = H.family_case(8, 40, 30, 1e3, 1e3, 0.3)
    nz32, b32 = nz.astype(np.float32), b.astype(np.float32)
    rl = M.RowLists(colptr, rowval, N)
    want, wst = BM.solve(rl, 1.0, -GAMMA, nz32, b32, 1e-6, MAXIT, precond=("block", 8))
    s = _solver(colptr, rowval, N, dtype=np.float32)
    s.set_preconditioner("block_jacobi", 8)
    got, st = _device_solve(s, nz32, b32, rtol=1e-6)
    assert wst["flags"] == 0 and st == wst and _same_bits(got, want)


# ---- 7. the switch leaves nothing behind ------------------------------------------------------------------------------------------------
def test_jacobi_after_block_jacobi_reproduces_a_fresh_solver():
    import test_cscsolve_model_cpu as HJ
    colptr, rowval, N, nz, b, gamma, J = HJ.make_case("lap5", 0.9)
    assert N == 300 * 200
    fresh, fst = _device_solve(_solver(colptr, rowval, N), nz, b, gamma, rtol=HJ.RTOL, maxit=HJ.MAXIT)
    assert fst["flags"] == 0
    s = _solver(colptr, rowval, N)
    s.set_preconditioner("block_jacobi", 5)
    used, ust = _device_solve(s, nz, b, gamma, rtol=HJ.RTOL, maxit=HJ.MAXIT)
    wantb, wstb = BM.solve(M.RowLists(colptr, rowval, N), 1.0, -gamma, nz, b, HJ.RTOL, HJ.MAXIT, precond=("block", 5))
    assert ust == wstb and _same_bits(used, wantb) and not _same_bits(used, fresh)
    s.set_preconditioner("jacobi")
    again, ast = _device_solve(s, nz, b, gamma, rtol=HJ.RTOL, maxit=HJ.MAXIT)
    assert ast == fst and _same_bits(again, fresh)
    s.set_preconditioner("block_jacobi", 32)                         # a larger size on the same solver: the buffers grow
    s.set_preconditioner("block_jacobi", 3)
    s.set_preconditioner("jacobi", None)
    again, ast = _device_solve(s, nz, b, gamma, rtol=HJ.RTOL, maxit=HJ.MAXIT)
    assert ast == fst and _same_bits(again, fresh)


# ---- 8. failure paths -------------------------------------------------------------------------------------------------------------------
def test_a_singular_or_nan_block_is_a_breakdown_not_a_fault():
    colptr, rowval, N, b, sing, nan, B = H.singular_and_nan_cases()
    s = _solver(colptr, rowval, N)
    s.set_preconditioner("block_jacobi", 4)
    for nz in (sing, nan):
        got, st = _device_solve(s, nz, b)
        assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(got))
        kept, stk = _device_solve(s, nz, b, keep=True)
        assert stk["flags"] == 2 and stk["iterations"] == 0 and np.array_equal(kept, np.zeros(N))
        want, bad = BM.block_inverses(colptr, rowval, N, 1.0, -GAMMA, nz, 4)
        got = s.block_inverses().cpu().numpy()
        # the arithmetic goes on behind the bad pivot: NaN where the model has NaN (the sign and payload of a NaN are no result of the
        # arithmetic and differ between the host and the device), the same bits -- Inf included -- everywhere else
        nan = np.isnan(want)
        print("bad block: %d NaN, %d Inf of %d" % (nan.sum(), np.isinf(want).sum(), want.size))
        assert bad and nan.any() and np.array_equal(np.isnan(got), nan)
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    # the same solver is clean again on the regular values
    colptr2, rowval2, nz2, N2, b2 = H.family_case(4, 12, 10, 1e3, 1e3, 0.0)
    want, wst = BM.solve(M.RowLists(colptr, rowval, N), 1.0, -GAMMA, nz2, b2, RTOL, MAXIT, precond=("block", 4))
    got, st = _device_solve(s, nz2, b2)
    assert st == wst and st["flags"] == 0 and _same_bits(got, want)


def test_dominant_tridiagonal_with_blocks_of_two_and_b_zero():
    import test_cscsolve_model_cpu as HJ
    colptr, rowval, N, nz, b, gamma, J = HJ.make_case("tridiag", 0.5)
    rl = M.RowLists(colptr, rowval, N)
    want, wst = BM.solve(rl, 1.0, -gamma, nz, b, RTOL, MAXIT, precond=("block", 2))
    _, jst = M.solve(rl, 1.0, -gamma, nz, b, RTOL, MAXIT)
    s = _solver(colptr, rowval, N)
    s.set_preconditioner("block_jacobi", 2)
    got, st = _device_solve(s, nz, b, gamma)
    assert st == wst and st["flags"] == 0 and st["iterations"] <= jst["iterations"] and _same_bits(got, want)
    got0, st0 = _device_solve(s, nz, np.zeros(N), gamma)
    assert st0 == {"flags": 0, "iterations": 0, "resid": 0.0, "bnorm": 0.0} and np.array_equal(got0, np.zeros(N))


# ---- 9. end to end ----------------------------------------------------------------------------------------------------------------------
REACT_DIFF = """
// nx x ny cells, m species per cell (the fastest index): diffusion per species to the four neighbouring cells, and a stiff reaction that
// couples the species of a cell non-symmetrically
struct ReactDiff {
    long long nx, ny, m;
    double k;
    template <class P> __device__ real_t operator()(long long r, const P &X) const
    {
        const long long cell = r / m, s = r - cell * m, j = cell / nx, i = cell - j * nx;
        const real_t c = (real_t)0.5 + (real_t)s / (real_t)(m - 1);
        const real_t dn = X(j > 0 ? r - nx * m : r), lf = X(i > 0 ? r - m : r), rt = X(i + 1 < nx ? r + m : r), up = X(j + 1 < ny ? r + nx * m : r);
        real_t lap = (j > 0 ? dn : (real_t)0) + (i > 0 ? lf : (real_t)0);
        lap = lap + (i + 1 < nx ? rt : (real_t)0);
        lap = lap + (j + 1 < ny ? up : (real_t)0);
        lap = lap - (real_t)4 * X(r);
        real_t acc = 0;
        for (long long t = 0; t < m; ++t) {
            const real_t xt = X(cell * m + t), d = (real_t)(s - t);
            const real_t w = (real_t)1 / ((real_t)1 + d * d) + (t > s ? (real_t)0.6 : (t < s ? (real_t)-0.6 : (real_t)0));
            acc = acc + w * (xt + ((real_t)0.5 * xt) * xt);
        }
        return c * lap - (real_t)k * acc;
    }
};
"""


def test_implicit_euler_step_on_a_reaction_diffusion_jacobian_the_library_stored():
    nx, ny, m, k = 24, 20, 6, 200.0
    colptr, rowval, _, N = BM.reaction_diffusion(nx, ny, m, 1.0, 10.0, 0.0, 0)          # (the pattern only)
    cp, rv = _dev((colptr + 1).astype(np.int32)), _dev((rowval + 1).astype(np.int32))
    colors, nc = fd.matrix_colors_device(N, N, cp, rv)
    plan = fd.make_plan_csc_device(N, N, cp, rv, colors, "forward", store_csc=True)
    f = fd.JitF(REACT_DIFF, "ReactDiff", N, N, params=struct.pack("qqqd", nx, ny, m, k))
    plan.set_lazy(f)
    x = _dev(np.random.default_rng(8).random(N) * 0.5)
    nzd = torch.full((rowval.size,), float("nan"), dtype=torch.float64, device="cuda")
    plan.jacobian(f, x, [nzd])
    assert not torch.isnan(nzd).any()
    # one implicit-Euler step x1 = x + y of x' = f(x) with h = 0.1: (I - h J(x)) y = h f(x), f(x) by the functor's own launcher
    h = GAMMA
    fx = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    assert f.fn(f.fctx, fx.data_ptr(), x.data_ptr(), 1, N, N, 0, N, 0, f.ctx.stream) == 0
    bd = h * fx
    b = bd.cpu().numpy()
    assert np.all(np.isfinite(b)) and np.abs(b).max() > 1.0                              # a stiff step: h |f| is not small
    s = fd.CscSolver((cp, rv, N), idx_base=1)
    s.set_options(RTOL, MAXIT)
    s.set_preconditioner("block_jacobi", m)
    y = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    s.solve(nzd, bd, y, 1.0, -h)                                                         # nzval and f(x) never left the device
    st = s.status()
    vals = nzd.cpu().numpy()
    res = H.true_residual(colptr, rowval, vals, N, 1.0, -GAMMA, y.cpu().numpy(), b)
    s.set_preconditioner("jacobi")
    yj = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    s.solve(nzd, bd, yj, 1.0, -h)
    stj = s.status()
    print("end to end: %d colours, block Jacobi flags %d iterations %d true residual %.3e | Jacobi flags %d iterations %d"
          % (nc, st["flags"], st["iterations"], res, stj["flags"], stj["iterations"]))
    assert st["flags"] == 0 and 1 <= st["iterations"] < MAXIT
    assert res <= 10 * RTOL
    want, wst = BM.solve(M.RowLists(colptr, rowval, N), 1.0, -GAMMA, vals, b, RTOL, MAXIT, precond=("block", m))
    assert st == wst and _same_bits(y.cpu().numpy(), want)


# ---- 10. the C client -------------------------------------------------------------------------------------------------------------------
def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "csc_precond_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "csc_precond_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "csc precond: PASS" in out.stdout, out.stdout
