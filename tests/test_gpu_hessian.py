"""The objective Hessian / gradient on the MI355X (fd_objective_compile / fd_hessian / fd_gradient): bit-identical to the
reference's loops when M = 1 (tests/hess_model.py restates src/hessians.jl:202-292 and src/gradients.jl:407-446), bit-identical to
the host exact model of the per-row contract when M > 1, the reference's own known answers, the three destinations, a Newton step
through the banded solver, launch counts and errors."""
import json
import os

import numpy as np
import pytest

import finitediff_jl_amd as fd
from finitediff_jl_amd import lib as L_
from finitediff_jl_amd import patterns as P

import hess_model as hm

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _i64(v):
    return np.int64(v).tobytes()


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _csc(M, N, cp0, rv0):
    return fd.SparseMatrixCSC(M, N, np.asarray(cp0) + 1, np.asarray(rv0) + 1)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _x(n, seed):
    x = np.random.default_rng(seed).standard_normal(n) * 2
    x[0] = 0.0                                    # absstep branch
    x[n // 2] = 0.0
    x[-1] = -abs(x[-1]) - 0.5
    return x


# ---- 1. the reference's setting: M = 1, dense support -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 7, 64, 257])
def test_dense_M1_hessian_and_gradient_are_the_reference_bit_for_bit(n, torch):
    f = fd.ObjectiveF(hm.POLYDIV_SRC, "PolyDiv", 1, n, params=_i64(n))
    phi = hm.phi_polydiv(n)
    x = _x(n, n)
    cache = fd.HessianCache(x)
    for relstep, absstep in ((None, None), (1e-3, 1e-6)):
        ref = hm.ref_hessian(phi, x, relstep=relstep, absstep=absstep)
        H = fd.finite_difference_hessian(f, x, cache, relstep=relstep, absstep=absstep)          # host arrays
        assert _bits_equal(H, ref), (n, relstep)
        xd = torch.as_tensor(x, device="cuda:0")
        Hd = torch.full((n, n), 7.0, dtype=torch.float64, device="cuda:0")
        fd.finite_difference_hessian_b(Hd, f, xd, cache, relstep=relstep, absstep=absstep)      # device arrays, enqueued
        assert _bits_equal(Hd.cpu().numpy(), ref), (n, relstep)
    for fdtype, dirs in (("forward", (1.0, -1.0)), ("central", (1.0,))):
        gc = fd.GradientCache(x, fdtype)
        for d in dirs:
            for relstep, absstep in ((None, None), (1e-4, 1e-8)):
                ref = hm.ref_gradient(phi, x, fdtype, relstep=relstep, absstep=absstep, dir=d)
                g = fd.finite_difference_gradient(f, x, gc, relstep=relstep, absstep=absstep, dir=d)
                assert _bits_equal(g, ref), (n, fdtype, d, relstep)
                gd = torch.zeros(n, dtype=torch.float64, device="cuda:0")
                fd.finite_difference_gradient_b(gd, f, torch.as_tensor(x, device="cuda:0"), gc, relstep=relstep, absstep=absstep, dir=d)
                assert _bits_equal(gd.cpu().numpy(), ref), (n, fdtype, d, relstep)


# ---- 2. known answers of the reference's tests, as one f (M = 1) and one row per coordinate (M = n, diagonal S) -------------------
@pytest.mark.parametrize("case", json.load(open(os.path.join(GOLD, "hessian_known_answers.json")))["cases"], ids=lambda c: c["name"])
def test_known_answers(case):
    x = np.array(case["x"], np.float64)
    n = x.size
    Href = np.array(case["H"])
    kind = hm.KNOWN_KINDS[case["name"]]
    for per in (0, 1):
        M = n if per else 1
        f = fd.ObjectiveF(hm.KNOWN_SRC, "Known", M, n, params=np.array([kind, n, per], np.int64).tobytes())
        S = _csc(n, n, np.arange(n + 1), np.arange(n)) if per else None
        H = fd.finite_difference_hessian(f, x, fd.HessianCache(x, S))
        if case["check"] == "exact":
            assert np.array_equal(H, Href), (per, H)
        elif case["check"] == "isapprox":
            assert np.linalg.norm(H - Href) <= case["tol"] * max(np.linalg.norm(H), np.linalg.norm(Href)), (per, H)
        else:
            assert np.max(np.abs(H - Href)) < case["tol"], (per, H)
        if per:
            off = ~np.eye(n, dtype=bool)
            assert np.all(H[off] == 0) and not np.signbit(H[off]).any()                     # structural zeros are exact +0.0


# ---- 3. sparse objectives against the host exact model -------------------------------------------------------------------------
def _sparse_cases():
    n = 100_000
    cp, rv = hm.chain_support(n)
    yield "chain", hm.CHAIN_SRC, "Chain", _i64(n), n, n, cp, rv, hm.phi_chain(n)
    nx, ny = 300, 200
    cp, rv = P.lap5_csc(nx, ny)
    yield "grid5", hm.GRID5_SRC, "Grid5", np.array([nx, ny], np.int64).tobytes(), nx * ny, nx * ny, cp - 1, rv - 1, hm.phi_grid5(nx, ny)
    M, N = 3000, 2000
    cp, rv = hm.randrows_support(M, N, N - 7)
    yield "random", hm.RANDROWS_SRC, "RandRows", _i64(N - 7), M, N, cp, rv, hm.phi_randrows(N - 7)


def _device_upper(cache, nz):
    """(i, j, value) of the upper entries of the CSC destination, sorted by (j, i); and the mirrored lower values"""
    Pm = cache.pattern()
    cp, rv = Pm.colptr - 1, Pm.rowval - 1
    col = np.repeat(np.arange(Pm.n, dtype=np.int64), np.diff(cp))
    up = rv <= col
    lo = rv > col
    o = np.lexsort((col[lo], rv[lo]))                 # (j, i) = (row, col) of the lower entries, sorted by j then i
    return rv[up], col[up], nz[up], col[lo][o], rv[lo][o], nz[lo][o]


@pytest.mark.parametrize("case", list(_sparse_cases()), ids=lambda c: c[0])
def test_sparse_objectives_are_the_exact_model_bit_for_bit(case, torch):
    name, src, typ, params, M, N, cp, rv, phi = case
    f = fd.ObjectiveF(src, typ, M, N, params=params)
    x = np.random.default_rng(7).standard_normal(N)
    x[::97] = 0.0
    S = _csc(M, N, cp, rv)
    cache = fd.HessianCache(x, S, dest="csc")
    Pm = cache.pattern()
    want = P.hessian_sparsity(S)
    assert np.array_equal(Pm.colptr, want.colptr) and np.array_equal(Pm.rowval, want.rowval)
    xd = torch.as_tensor(x, device="cuda:0")
    nz = torch.zeros(Pm.rowval.size, dtype=torch.float64, device="cuda:0")
    fd.finite_difference_hessian_b(nz, f, xd, cache)
    nz = nz.cpu().numpy()
    i, j, v, li, lj, lv = _device_upper(cache, nz)
    mi, mj, mh = hm.hessian_entries(phi, x, M, N, cp, rv)
    assert np.array_equal(i, mi) and np.array_equal(j, mj)
    assert _bits_equal(v, mh), name
    off = mi != mj
    assert np.array_equal(li, mi[off]) and np.array_equal(lj, mj[off]) and _bits_equal(lv, mh[off])        # mirrored, same bits
    for fdtype in ("forward", "central"):
        gd = torch.zeros(N, dtype=torch.float64, device="cuda:0")
        fd.finite_difference_gradient_b(gd, f, xd, fd.GradientCache(x, fdtype, S))
        assert _bits_equal(gd.cpu().numpy(), hm.gradient(phi, x, M, N, fdtype, cp, rv)), (name, fdtype)


def _small_cases():
    n = 120
    cp, rv = hm.chain_support(n)
    yield "chain", hm.CHAIN_SRC, "Chain", _i64(n), n, n, cp, rv, hm.phi_chain(n)
    nx, ny = 6, 5                    # (the whole-f reference's own rounding grows with f: kept small)
    cp, rv = P.lap5_csc(nx, ny)
    yield "grid5", hm.GRID5_SRC, "Grid5", np.array([nx, ny], np.int64).tobytes(), nx * ny, nx * ny, cp - 1, rv - 1, hm.phi_grid5(nx, ny)
    M, N = 150, 100
    cp, rv = hm.randrows_support(M, N, N - 5)
    yield "random", hm.RANDROWS_SRC, "RandRows", _i64(N - 5), M, N, cp, rv, hm.phi_randrows(N - 5)


@pytest.mark.parametrize("case", list(_small_cases()), ids=lambda c: c[0])
def test_sparse_objectives_agree_with_the_dense_reference(case):
    # n <= 300: the reference's whole-f loops on f = sum_r phi_r, to rounding (the per-row sums are the more accurate)
    name, src, typ, params, M, N, cp, rv, phi = case
    f = fd.ObjectiveF(src, typ, M, N, params=params)
    x = np.random.default_rng(11).standard_normal(N)

    def whole(r, get):
        s = np.zeros(np.shape(r))
        for k in range(M):
            s = s + phi(np.full(np.shape(r), k, np.int64), get)
        return s
    H = fd.finite_difference_hessian(f, x, fd.HessianCache(x, _csc(M, N, cp, rv)))
    R = hm.ref_hessian(whole, x)
    assert np.max(np.abs(H - R)) <= 1e-6 * np.max(np.abs(R)), name
    assert _bits_equal(H, hm.hessian(phi, x, M, N, cp, rv)[0])


# ---- 4. destinations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["chain", "grid5"])
def test_destinations_hold_the_same_bits(which, torch):
    if which == "chain":
        n = 333
        cp, rv = hm.chain_support(n)
        f = fd.ObjectiveF(hm.CHAIN_SRC, "Chain", n, n, params=_i64(n))
    else:
        nx, ny = 9, 7
        n = nx * ny
        cp, rv = P.lap5_csc(nx, ny)
        cp, rv = cp - 1, rv - 1
        f = fd.ObjectiveF(hm.GRID5_SRC, "Grid5", n, n, params=np.array([nx, ny], np.int64).tobytes())
    S = _csc(n, n, cp, rv)
    x = np.random.default_rng(5).standard_normal(n)
    xd = torch.as_tensor(x, device="cuda:0")
    dense = fd.HessianCache(x, S, dest="dense")
    Hd = torch.full((n, n), np.nan, dtype=torch.float64, device="cuda:0")       # (every slot is written: P or +0.0)
    fd.finite_difference_hessian_b(Hd, f, xd, dense)
    Hd = Hd.cpu().numpy()
    csc = fd.HessianCache(x, S, dest="csc")
    Pm = csc.pattern()
    nz = torch.full((Pm.rowval.size,), np.nan, dtype=torch.float64, device="cuda:0")
    fd.finite_difference_hessian_b(nz, f, xd, csc)
    H_csc = P.csc_to_dense(n, n, Pm.colptr, Pm.rowval, nz.cpu().numpy())
    assert _bits_equal(H_csc, Hd)
    inP = H_csc != 0
    inP[Pm.rowval - 1, np.repeat(np.arange(n), np.diff(Pm.colptr))] = True
    assert np.all(Hd[~inP] == 0) and not np.signbit(Hd[~inP]).any()
    bw = dense.info(L_.HESS_INFO_BANDWIDTH)
    assert bw == (2 if which == "chain" else 2 * nx)
    for band in (bw, bw + 2):
        c = fd.HessianCache(x, S, dest="banded", band=band)
        w = 2 * band + 1
        data = torch.full((n, w), np.nan, dtype=torch.float64, device="cuda:0").t()       # (2 band + 1) x n column-major
        fd.finite_difference_hessian_b(fd.BandedMatrix(data, n, band, band), f, xd, c)
        Hb = P.banded_to_dense(data.cpu().numpy(), n, n, band, band)
        assert _bits_equal(Hb, Hd), band
        raw = data.cpu().numpy()
        assert not np.isnan(raw).any() and not np.signbit(raw[raw == 0]).any()        # out-of-matrix / outside-P slots: +0.0
    with pytest.raises(fd.lib.FdError) as e:
        fd.HessianCache(x, S, dest="banded", band=bw - 1)
    assert e.value.code == 1                                                          # FD_ERR_ARG


# ---- 5. a Newton step of optimisation on the device ----------------------------------------------------------------------------
def test_newton_step_through_the_banded_solver(torch):
    import scipy.linalg
    n = 1_000_000
    cp, rv = hm.chain_support(n)
    S = _csc(n, n, cp, rv)
    f = fd.ObjectiveF(hm.CHAIN_SRC, "Chain", n, n, params=_i64(n))
    x = torch.as_tensor(np.random.default_rng(2).uniform(-1.5, 1.5, n), device="cuda:0")
    x0 = x.clone()
    hc = fd.HessianCache(x, S, dest="banded")
    assert hc.band == 2
    data = torch.zeros((n, 5), dtype=torch.float64, device="cuda:0").t()
    H = fd.BandedMatrix(data, n, 2, 2)
    g = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    fd.finite_difference_hessian_b(H, f, x, hc)
    fd.finite_difference_gradient_b(g, f, x, fd.GradientCache(x, "central", S))
    solver = fd.BandedSolver(n, 2, 2, "banded")
    d = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    rhs = -g
    solver.solve(H, rhs, d, alpha=0.0, beta=1.0)
    assert solver.status() == 0                     # diagonally dominant: the default policy accepts it
    assert torch.equal(x, x0)
    ab, b = data.cpu().numpy(), rhs.cpu().numpy()
    want = scipy.linalg.solve_banded((2, 2), ab, b)
    got = d.cpu().numpy()
    assert np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))


# ---- 6. launch counts ---------------------------------------------------------------------------------------------------------
def test_launch_counts(torch):
    n = 5000
    cp, rv = hm.chain_support(n)
    S = _csc(n, n, cp, rv)
    f = fd.ObjectiveF(hm.CHAIN_SRC, "Chain", n, n, params=_i64(n))
    x = torch.as_tensor(np.linspace(-1, 1, n), device="cuda:0")
    hc = fd.HessianCache(x, S, dest="csc")
    nz = torch.zeros(hc.info(L_.HESS_INFO_NNZ), dtype=torch.float64, device="cuda:0")
    g = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    for kind, call, per in (("hessian", lambda: fd.finite_difference_hessian_b(nz, f, x, hc), 2),
                            ("forward", lambda: fd.finite_difference_gradient_b(g, f, x, fd.GradientCache(x, "forward", S)), 2),
                            ("central", lambda: fd.finite_difference_gradient_b(g, f, x, fd.GradientCache(x, "central", S)), 1)):
        before = f.launches
        for _ in range(3):
            call()
        assert f.launches - before == 3 * per, kind


# ---- 7. errors and NaN steps ----------------------------------------------------------------------------------------------------
def test_errors():
    L = fd.lib.load()
    with pytest.raises(fd.lib.FdError) as e:
        fd.ObjectiveF("struct Bad { template <class P> __device__ real_t operator()(long long r, const P &X) const { return X(r) +; } };",
                      "Bad", 4, 4)
    assert e.value.code == 1 and L.fd_f_compile_log()             # FD_ERR_ARG, the compiler's messages kept
    cp, rv = hm.chain_support(10)
    f11 = fd.ObjectiveF(hm.CHAIN_SRC, "Chain", 11, 11, params=_i64(11))
    x = np.zeros(10)
    with pytest.raises(fd.lib.FdError) as e:
        fd.finite_difference_hessian(f11, x, fd.HessianCache(x, _csc(10, 10, cp, rv)))
    assert e.value.code == 2                                       # FD_ERR_SHAPE
    f10 = fd.ObjectiveF(hm.CHAIN_SRC, "Chain", 10, 10, params=_i64(10))
    with pytest.raises(fd.lib.FdError) as e:
        fd.finite_difference_gradient(f10, x, fd.GradientCache(x, "complex", _csc(10, 10, cp, rv)))
    assert e.value.code == 3                                       # FD_ERR_UNSUPPORTED


@pytest.mark.parametrize("which", ["chain", "random"])
def test_nan_coordinate_poisons_what_the_model_poisons(which):
    if which == "chain":
        n = M = 30
        cp, rv = hm.chain_support(n)
        f = fd.ObjectiveF(hm.CHAIN_SRC, "Chain", n, n, params=_i64(n))
        phi = hm.phi_chain(n)
    else:
        M, n = 60, 40
        cp, rv = hm.randrows_support(M, n, n - 3)
        f = fd.ObjectiveF(hm.RANDROWS_SRC, "RandRows", M, n, params=_i64(n - 3))
        phi = hm.phi_randrows(n - 3)
    S = _csc(M, n, cp, rv)
    x = np.random.default_rng(9).standard_normal(n)
    x[7] = np.nan
    H = fd.finite_difference_hessian(f, x, fd.HessianCache(x, S))
    Hm, _ = hm.hessian(phi, x, M, n, cp, rv)
    assert np.isnan(H).any() and not np.isnan(H).all()
    assert np.array_equal(np.isnan(H), np.isnan(Hm)) and _bits_equal(np.nan_to_num(H), np.nan_to_num(Hm))
    for fdtype in ("forward", "central"):
        g = fd.finite_difference_gradient(f, x, fd.GradientCache(x, fdtype, S))
        gm = hm.gradient(phi, x, M, n, fdtype, cp, rv)
        assert np.array_equal(np.isnan(g), np.isnan(gm)) and _bits_equal(np.nan_to_num(g), np.nan_to_num(gm))
