"""CPU checks of the objective Hessian / gradient: the Hessian pattern P = pattern(S^T S) against scipy, the host exact model against an
independent restatement of the reference's loops (M = 1: bit for bit), and the new C ABI symbols (declared, exported, and failing
loudly without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P

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
