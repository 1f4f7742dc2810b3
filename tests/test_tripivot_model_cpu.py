"""The numpy model of the pivoted tridiagonal solve (tests/tri_pivot_model.py) against SciPy's pivoted banded LU refined in extended
precision: accuracy on four non-dominant families, coverage of both pivot choices on every level, and the failure paths.  No GPU:
tests/test_gpu_tripivot.py then asks the device for the model's bits.

The accuracy assertion is  ||y - y_ref||_inf <= F * max(E_lapack, eps * ||y_ref||_inf),  F = 4 x the model's worst ratio of the family
over tri_pivot_model.SIZES (MEASURED below; profiles/solver_accuracy_pivot.md, rewritten by `python tests/test_tripivot_model_cpu.py`),
capped at 1024.  The factor 4 is there because other seeds move the ratio by small factors."""
import os

import numpy as np
import pytest

import tri_pivot_model as M
from solve_model import refined_reference

EPS, MEASURED, F_CAP, bound_factor, degenerate_11 = M.EPS, M.MEASURED, M.F_CAP, M.bound_factor, M.degenerate_11


def ratio_of(name, N):
    dl, d, du, rhs = M.family(name, N)
    r = M.piv_solve(dl, d, du, rhs)
    y_ref, e_lapack = refined_reference(M.system_of(dl, d, du, rhs, 0.0, 1.0))
    err = float(np.max(np.abs(r.y.astype(np.longdouble) - y_ref)))
    return r, err / max(e_lapack, EPS * float(np.max(np.abs(y_ref))))


def test_the_cap_is_a_condition_the_measured_factors_meet():
    assert all(4.0 * v <= F_CAP for v in MEASURED.values())


@pytest.mark.parametrize("name", M.FAMILIES)
def test_model_accuracy_against_refined_pivoted_lu(name):
    for N in M.family_sizes(name):
        r, ratio = ratio_of(name, N)
        print("%-9s N = %6d  ratio %.3g  status %d" % (name, N, ratio, r.status))
        assert not (r.status & M.BAD_PIVOT), (name, N)
        assert np.all(np.isfinite(r.y)), (name, N)
        assert ratio <= bound_factor(name), (name, N, ratio)


def test_level_schedule():
    assert M.piv_levels(10 ** 7) == [10 ** 7, 2500000, 625000, 156250, 39064, 9766, 2442, 612]
    assert M.piv_levels(70001) == [70001, 17501, 4376, 1094]      # (8750 chunks of 8 and one of m = 1: 2 * 8750 + 1)
    assert M.piv_levels(2048) == [2048] and M.piv_levels(2049) == [2049, 513] and M.piv_levels(2050) == [2050, 514]
    # last chunks of m = 1, 2, 3 and 8 rows on the first two levels of the size list
    seen = set()
    for N in M.SIZES:
        for n in M.piv_all_levels(N)[:2]:
            if n > M.KCHUNK:
                seen.add(n - M.KCHUNK * (-(-n // M.KCHUNK) - 1))
    assert {1, 2, 3, 8} <= seen


def test_both_pivot_choices_on_every_level():
    r = M.piv_solve(*M.family("gauss", 70001))
    assert len(r.swaps) == len(M.piv_all_levels(70001))
    for lv, sw in enumerate(r.swaps):
        assert sw.size and sw.any() and not sw.all(), lv
    r = M.piv_solve(*M.family("advect", 2057))
    assert r.swaps[0].any()


def test_zero_matrix_gives_bit_2_and_nan():
    N = 70
    r = M.piv_solve(np.zeros(N - 1), np.zeros(N), np.zeros(N - 1), np.ones(N), alpha=0.0, beta=1.0)
    assert r.status & M.BAD_PIVOT and np.all(np.isnan(r.y))


def test_shared_row_degeneracy_ends_in_bit_2_not_in_a_wrong_answer():
    dl, d, du, rhs = degenerate_11()
    A = np.diag(d) + np.diag(dl, -1) + np.diag(du, 1)
    assert abs(np.linalg.det(A)) > 1.0                      # the matrix itself is regular
    r = M.piv_solve(dl, d, du, rhs)
    assert r.status & M.BAD_PIVOT and np.all(np.isnan(r.y))


def test_dominant_system_never_swaps_on_level_0():
    N = 2057
    rng = np.random.default_rng(3)
    dl, du = rng.uniform(-1, 1, N - 1), rng.uniform(-1, 1, N - 1)
    d = 2.5 + rng.random(N)
    rhs = rng.standard_normal(N)
    r = M.piv_solve(dl, d, du, rhs)
    assert r.status == 0 and not r.swaps[0].any()
    A = np.diag(d) + np.diag(dl, -1) + np.diag(du, 1)
    assert np.max(np.abs(A @ r.y - rhs)) <= 64 * EPS * np.max(np.abs(rhs))


def test_csc_layout_differs_from_diagonals_only_in_the_sign_of_absent_zeros():
    dl, d, du, rhs = M.family("gauss", 2057)
    a0 = M.level0_rows(dl, d, du, rhs, 1.0, -0.5, "diagonals")
    a1 = M.level0_rows(dl, d, du, rhs, 1.0, -0.5, "csc")
    assert all(np.array_equal(u, v) for u, v in zip(a0, a1))
    assert not np.signbit(a0[0][0]) and np.signbit(a1[0][0]) and np.signbit(a1[2][-1])


def test_the_switch_reaches_every_layer():
    import re
    import finitediff_jl_amd as fd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fdjac.h")).read()
    for sym in ("fd_tridiag_solver_set_pivoting", "fd32_tridiag_solver_set_pivoting"):
        assert re.search(r"^int %s\(" % sym, hdr, re.M) and sym in fd.lib.EXPORTS, sym
    assert "fd_tridiag_solver_set_pivoting" in fd.lib.TYPED
    assert fd.TridiagSolver.set_pivoting.__doc__ and "bit 2" in fd.TridiagSolver.status.__doc__
    shim = open(os.path.join(root, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    assert '"tridiag_solver_set_pivoting"' in shim and "set_pivoting!" in shim
    assert os.path.exists(os.path.join(root, "examples", "tridiag_pivot_client.c"))
    for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        assert "fd_tridiag_solver_set_pivoting" in open(os.path.join(root, doc)).read(), doc
    src = open(os.path.join(root, "finitediff.jl_amd", "csrc", "fdjac_solve.hip")).read()
    assert "constexpr int kPivTop = kTriTileRows;" in src and M.KPIVTOP == 2048 and M.KCHUNK == 8


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ["# Pivoted tridiagonal solve: the model's error against refined pivoted LU", "",
             "`python tests/test_tripivot_model_cpu.py` (CPU, numpy model of csrc/fdjac_solve.hip's k_tripiv_* kernels; the device returns the",
             "same bits, tests/test_gpu_tripivot.py).  ratio = ||y - y_ref||_inf / max(E_lapack, eps ||y_ref||_inf); y_ref = SciPy's banded LU",
             "refined in extended precision, E_lapack = that LU's own error.  The tests assert F = 4 x the family's worst ratio (cap 1024).", "",
             "| family | N | ratio | E_lapack | status |", "|---|---|---|---|---|"]
    worst = {}
    for name in M.FAMILIES:
        for N in M.family_sizes(name):
            dl, d, du, rhs = M.family(name, N)
            r, ratio = ratio_of(name, N)
            _y, e = refined_reference(M.system_of(dl, d, du, rhs, 0.0, 1.0))
            lines.append("| %s | %d | %.3g | %.3g | %d |" % (name, N, ratio, e, r.status))
            if ratio > worst.get(name, (0.0, 0))[0]:
                worst[name] = (ratio, N)
    lines += ["", "| family | worst ratio | at N | asserted F |", "|---|---|---|---|"]
    for name in M.FAMILIES:
        lines.append("| %s | %.3g | %d | %.3g |" % (name, worst[name][0], worst[name][1], min(4.0 * MEASURED[name], F_CAP)))
        assert worst[name][0] <= MEASURED[name], (name, worst[name])
    open(os.path.join(root, "profiles", "solver_accuracy_pivot.md"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
