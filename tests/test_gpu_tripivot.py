"""The pivoted tridiagonal solve (fd_tridiag_solver_set_pivoting; csrc/fdjac_solve.hip, k_tripiv_*) on the device: y and the status word
EQUAL the numpy model of tests/tri_pivot_model.py bit for bit -- four non-dominant families, sizes around every chunk / tile / level
boundary and 10^6 + 3, both layouts, both element types, two shifts --, twice on one solver; the gap itself (the default path refuses
`advect`, the pivoted one solves it within the model's accuracy bound); the toggle; the failure paths; the refusals of the sharded
entry points; end to end behind a run-time compiled advection functor through a tridiagonal and a CSC plan; the C client."""
import os
import struct
import subprocess

import numpy as np
import pytest

import finitediff_jl_amd as fd
import tri_pivot_model as M
from finitediff_jl_amd import patterns as P
from solve_model import refined_reference
from tri_pivot_model import EPS, bound_factor, degenerate_11

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = [(0.0, 1.0), (1.0, -0.5)]
BIG = 10 ** 6 + 3
FD_ERR_UNSUPPORTED = 3


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _csc_nzval(dl, d, du):
    N = d.size
    if N == 1:
        return d.copy()
    out = np.empty(3 * N - 2, d.dtype)
    j = np.arange(N)
    out[np.where(j > 0, 3 * j, 0)] = d
    out[3 * j[1:] - 1] = du
    out[3 * j[:-1] + 1] = dl
    return out


def _J(dl, d, du, layout):
    if layout == "diagonals":
        return fd.Tridiagonal(_dev(dl), _dev(d), _dev(du))
    return [_dev(_csc_nzval(dl, d, du))]


def _solve(solver, J, b, alpha, beta):
    keep = b.clone()
    y = torch.full((b.numel(),), float("nan"), dtype=b.dtype, device="cuda")
    solver.solve(J, b, y, alpha, beta)
    st = solver.status()
    assert torch.equal(b, keep)
    return y.cpu().numpy(), st


def _same_bits(got, want):
    if np.all(np.isnan(want)):
        return bool(np.all(np.isnan(got)))
    iv = np.int64 if got.dtype == np.float64 else np.int32
    return got.dtype == want.dtype and np.array_equal(got.view(iv), want.view(iv))


def _sizes(name):
    return M.family_sizes(name) + [BIG + 1 if name == "zero_diag" else BIG]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", M.FAMILIES)
def test_bits_equal_the_model(name, shift, dtype):
    alpha, beta = shift
    for N in _sizes(name):
        dl, d, du, rhs = M.family(name, N, dtype=dtype)
        for layout in ("diagonals", "csc"):
            want = M.piv_solve(dl, d, du, rhs, alpha, beta, layout, dtype)
            solver = fd.TridiagSolver(N, layout, dtype=dtype)
            solver.set_pivoting(True)
            J, b = _J(dl, d, du, layout), _dev(rhs)
            y, st = _solve(solver, J, b, alpha, beta)
            label = (name, N, layout, np.dtype(dtype).name, shift)
            assert st == want.status, (label, st, want.status)
            assert _same_bits(y, want.y), (label, int(np.sum(y != want.y)))
            y2, st2 = _solve(solver, J, b, alpha, beta)            # twice on one solver: the same bits
            assert st2 == st and _same_bits(y2, y), label


def test_the_gap_itself_refused_without_pivoting_solved_with_it():
    N = 16385
    dl, d, du, rhs = M.family("advect", N)
    y_ref, e_lapack = refined_reference(M.system_of(dl, d, du, rhs, 0.0, 1.0))
    tol = bound_factor("advect") * max(e_lapack, EPS * float(np.max(np.abs(y_ref))))
    for layout in ("diagonals", "csc"):
        solver = fd.TridiagSolver(N, layout)
        J, b = _J(dl, d, du, layout), _dev(rhs)
        y, st = _solve(solver, J, b, 0.0, 1.0)
        assert st == 1 and np.all(np.isnan(y))                  # today's behaviour, unchanged
        solver.set_pivoting(True)
        y, st = _solve(solver, J, b, 0.0, 1.0)
        err = float(np.max(np.abs(y.astype(np.longdouble) - y_ref)))
        print("advect N=%d @%s err=%.3e tol=%.3e" % (N, layout, err, tol))
        assert st & 1 and not st & 4 and np.all(np.isfinite(y))
        assert err <= tol, (layout, err, tol)


def test_toggle_restores_the_default_path_bit_for_bit():
    N = 70001
    rng = np.random.default_rng(5)
    dl, du, d, rhs = rng.uniform(-1, 1, N - 1), rng.uniform(-1, 1, N - 1), 2.5 + rng.random(N), rng.standard_normal(N)
    for layout in ("diagonals", "csc"):
        J, b = _J(dl, d, du, layout), _dev(rhs)
        plain, st0 = _solve(fd.TridiagSolver(N, layout), J, b, 0.0, 1.0)
        solver = fd.TridiagSolver(N, layout)
        solver.set_pivoting(True)
        piv, st1 = _solve(solver, J, b, 0.0, 1.0)
        assert st0 == 0 and st1 == 0
        assert _same_bits(piv, M.piv_solve(dl, d, du, rhs, 0.0, 1.0, layout).y)
        solver.set_pivoting(False)
        back, st2 = _solve(solver, J, b, 0.0, 1.0)
        assert st2 == 0 and _same_bits(back, plain)


@pytest.mark.parametrize("N", [70, 2057, 16386])
def test_zero_matrix_gives_bit_2_and_nan_whatever_the_policy(N):
    z, rhs = np.zeros(N), np.ones(N)
    for layout in ("diagonals", "csc"):
        solver = fd.TridiagSolver(N, layout)
        solver.set_pivoting(True)
        solver.set_policy(True)
        y, st = _solve(solver, _J(z[:-1], z, z[:-1], layout), _dev(rhs), 0.0, 1.0)
        assert st & 4 and np.all(np.isnan(y)), (layout, st)


def test_shared_row_degeneracy_ends_in_bit_2():
    dl, d, du, rhs = degenerate_11()
    solver = fd.TridiagSolver(11, "diagonals")
    solver.set_pivoting(True)
    y, st = _solve(solver, _J(dl, d, du, "diagonals"), _dev(rhs), 0.0, 1.0)
    assert st == M.piv_solve(dl, d, du, rhs).status and st & 4 and np.all(np.isnan(y))


def test_sharded_entry_points_are_unsupported_with_pivoting_on():
    N = 5003
    dl, d, du, rhs = M.family("advect", N)
    window = fd.TridiagSolver(N, "diagonals", rows=(0, 2500))
    window.set_pivoting(True)
    Jw, bw = fd.Tridiagonal(_dev(dl[:2500]), _dev(d[:2500]), _dev(du[:2499])), _dev(rhs[:2500])
    y = torch.zeros(2500, dtype=torch.float64, device="cuda")
    packets = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    with pytest.raises(fd.lib.FdError) as e:
        window.solve(Jw, bw, y, 0.0, 1.0)
    assert e.value.code == FD_ERR_UNSUPPORTED
    whole = fd.TridiagSolver(N, "diagonals")
    whole.set_pivoting(True)
    J, b = _J(dl, d, du, "diagonals"), _dev(rhs)
    yw = torch.zeros(N, dtype=torch.float64, device="cuda")
    for s, args in ((window, (Jw, bw)), (whole, (J, b))):
        with pytest.raises(fd.lib.FdError) as e:
            s.interface(*args, packets[0], 0.0, 1.0)
        assert e.value.code == FD_ERR_UNSUPPORTED
        with pytest.raises(fd.lib.FdError) as e:
            s.finish(*args, packets, 0, 2, y if s is window else yw, 0.0, 1.0)
        assert e.value.code == FD_ERR_UNSUPPORTED
    assert torch.count_nonzero(y).item() == 0 and torch.count_nonzero(packets).item() == 0          # nothing was launched
    window.set_pivoting(False)                               # and off again: the sharded pieces work as before
    window.interface(Jw, bw, packets[0], 1.0, -0.01)


ADVECT = """
// du/dt = -c du/dx, central differences, plus a weak nonlinear reaction term: J has a (nearly) zero diagonal and -+k off it
struct Advect {
    long long n;
    double k;
    template <class P> __device__ real_t operator()(long long i, const P &X) const
    {
        const real_t xi = X(i), xm = X(i > 0 ? i - 1 : i), xp = X(i + 1 < n ? i + 1 : i);
        const real_t a = i > 0 ? xm : (real_t)0, b = i + 1 < n ? xp : (real_t)0;
        return (real_t)k * (a - b) + (real_t)0.001 * (xi * xi);
    }
};
"""


@pytest.mark.parametrize("storage", ["tridiagonal", "csc"])
def test_end_to_end_behind_a_compiled_advection_functor(storage):
    N, k, gamma = 2057, 3.0, 0.5                             # gamma c / h = 2 gamma k = 3
    x = _dev(np.random.default_rng(7).random(N))
    f = fd.JitF(ADVECT, "Advect", N, N, params=struct.pack("qd", N, k))
    colors = P.cyclic_colors(N, 3)
    if storage == "csc":
        cp, rv = P.tridiag_csc(N)
        Jp = fd.SparseMatrixCSC(N, N, cp, rv, None)
        outs = [_dev(np.full(rv.size, np.nan))]
        plan = fd.make_plan(Jp, Jp, colors, "central")
    else:
        Jp = fd.Tridiagonal(None, torch.empty(N, dtype=torch.float64, device="cuda"), None)
        outs = [_dev(np.full(N - 1, np.nan)), _dev(np.full(N, np.nan)), _dev(np.full(N - 1, np.nan))]
        plan = fd.make_plan(Jp, None, colors, "central")
    plan.jacobian(f, x, outs)
    rhs = np.random.default_rng(8).standard_normal(N)
    solver = fd.TridiagSolver(N, "csc" if storage == "csc" else "diagonals")
    b = _dev(rhs)
    y, st = _solve(solver, outs, b, 1.0, -gamma)             # on the values where the plan left them
    assert st == 1 and np.all(np.isnan(y))
    solver.set_pivoting(True)
    y, st = _solve(solver, outs, b, 1.0, -gamma)
    assert st == 1 and np.all(np.isfinite(y))
    if storage == "csc":
        nz = outs[0].cpu().numpy()
        j = np.arange(N)
        d, du, dl = nz[np.where(j > 0, 3 * j, 0)], nz[3 * j[1:] - 1], nz[3 * j[:-1] + 1]
    else:
        dl, d, du = [o.cpu().numpy() for o in outs]
    assert np.max(np.abs(d)) < 0.01 and np.min(np.abs(dl)) > 2.9          # the advection Jacobian: no dominance in I - gamma J
    y_ref, e_lapack = refined_reference(M.system_of(dl, d, du, rhs, 1.0, -gamma))
    tol = bound_factor("advect") * max(e_lapack, EPS * float(np.max(np.abs(y_ref))))
    err = float(np.max(np.abs(y.astype(np.longdouble) - y_ref)))
    print("end to end @%s err=%.3e tol=%.3e" % (storage, err, tol))
    assert err <= tol, (err, tol)
    assert _same_bits(y, M.piv_solve(dl, d, du, rhs, 1.0, -gamma, "csc" if storage == "csc" else "diagonals").y)


def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "tridiag_pivot_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tridiag_pivot_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pivoting off: status 1, y NaN" in out.stdout and "pivoting on: status 1," in out.stdout, out.stdout
    assert "tridiag pivot: PASS" in out.stdout, out.stdout
