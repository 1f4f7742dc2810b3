"""Storing kernels against the exact host model (tests/exact_model.py), bit for bit: k_f_tridiag_store_wave (Float64 two columns per
lane, Float32 four) into CSC / Banded / Tridiagonal, the fused step k_f_tridiag_fused, the hand-over path, k_f_stencil5_store_wave
(Float64) and k_f_stencil5_store_wave4 (Float32) -- at small and ragged sizes, with signed zeros, cancelling rows, step sizes at the
edges of div_shared's range, sums of squares that overflow or underflow (the scaled norm), subnormals and NaN / Inf coordinates.
More than kRegColors = 8 colours (per-colour lists, k_eps_finalize), the single-workgroup small-problem launch and complex-valued
x (the (re, im) pair branch of the reductions) take the same operands.  Every case asserts which path ran.  The step sizes equal the model's bits where the plain sum stands, and lie within 4 ulps of
mpmath where the scaled norm is taken (the stored values are then checked against the model evaluated at the device's step sizes)."""
import numpy as np
import pytest

import exact_model as X
from exact_operands import operands as _operands
from finitediff_jl_amd import patterns as P
import finitediff_jl_amd as fd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _ulps(a, b):
    it = np.int64 if a.dtype == np.float64 else np.int32
    return np.abs(a.view(it).astype(np.int64) - b.view(it).astype(np.int64))


CASES64 = ["ordinary", "signed_zeros", "cancel", "eps_2p100_in", "eps_2p100_out", "eps_2m100_in", "eps_2m100_out", "num_2p800",
           "huge_range", "tiny_1e-200", "subnormal", "nan_inf"]
CASES32 = ["ordinary", "signed_zeros", "f32_huge", "f32_subnormal", "nan_inf"]


def _check(plan, outs_dev, want_outs, x, c0, C, fdtype, rel, ab, dir, dtype, f, defined_order=True, f_in=None):
    """The step sizes (bits, or 4 ulps + mpmath semantics after the scaled norm), then every stored value against the model.
    defined_order=False: a reduction with a summation order of its own (more than kRegColors = 8 colours, the single-workgroup
    small-problem launch) -- its plain sums are within 4 ulps of the model's, NaN where the model's are.  f_in: the caller's f(x) of
    a forward difference, which the model subtracts as it is given."""
    got_eps = plan.epsilons().astype(dtype)
    eps, scaled = X.epsilons(x, c0, C, fdtype, relstep=rel, absstep=ab, dir=dir, dtype=dtype)
    plain = ~scaled
    if defined_order:
        ok = X.same_bits(got_eps[plain], eps[plain])
    else:
        fin = np.isfinite(eps[plain])
        ok = (np.isnan(got_eps[plain]) == np.isnan(eps[plain])) & (~fin | (_ulps(got_eps[plain], eps[plain]) <= 4))
    assert ok.all(), ("eps", got_eps, eps)
    if scaled.any():
        assert (_ulps(got_eps[scaled], eps[scaled]) <= 4).all(), ("scaled eps", got_eps, eps)
    D = X.colour_values(f, x, c0, C, got_eps, fdtype, f_in=f_in)
    for o, lay in zip(outs_dev, want_outs(D)):
        g = o.cpu().numpy()
        m = X.same_bits(g, lay)
        assert m.all(), (int((~m).sum()), np.nonzero(~m)[0][:6].tolist(), g[~m][:6].tolist(), lay[~m][:6].tolist())


def _tridiag_storage(kind, N, dtype):
    t = torch.float64 if dtype == np.float64 else torch.float32
    if kind == "csc":
        cp, rv = P.tridiag_csc(N)
        return fd.SparseMatrixCSC(N, N, cp, rv, torch.full((rv.size,), float("nan"), dtype=t, device="cuda"))
    if kind == "banded":
        return fd.BandedMatrix(torch.full((3 * N,), float("nan"), dtype=t, device="cuda"), N, 1, 1)
    return fd.Tridiagonal(*(torch.full((n,), float("nan"), dtype=t, device="cuda") for n in (max(N - 1, 0), N, max(N - 1, 0))))


def _tridiag_outs(J):
    if isinstance(J, fd.SparseMatrixCSC):
        return [J.nzval]
    if isinstance(J, fd.BandedMatrix):
        return [J.data]
    return [J.dl, J.d, J.du]


def _tridiag_layout(kind, N, c0):
    if kind == "csc":
        cp, rv = P.tridiag_csc(N)
        return lambda D: [X.to_csc(D, c0, cp, rv)]
    if kind == "banded":
        return lambda D: [X.to_banded(D, c0, N, N, 1, 1)]
    return lambda D: list(X.to_tridiagonal(D, c0, N))


def _run_tridiag(monkeypatch, N, C, shift, kind, dtype, fdtype, case, dir=1.0, path="store", family="tridiag_nl"):
    """path: "store" (the storing launch after the step-size launch), "fused" (one launch), "handover" (k_perturb + f! +
    decompression), "small" (hand-over behind the single-workgroup step-size launch).  Which one ran is asserted."""
    monkeypatch.setenv("FDJAC_SMALL", "1" if path == "small" else "0")     # otherwise the defined two-level order at every N
    monkeypatch.setenv("FDJAC_LAZY_STORE", "1" if path in ("store", "fused") else "0")
    colors = ((np.arange(N) + shift) % C + 1).astype(np.int64)
    c0 = colors - 1
    x, rel, ab = _operands(case, N, C, dtype, N * 7 + C)
    J = _tridiag_storage(kind, N, dtype)
    plan = fd.make_plan(J, J, colors, fdtype, dtype=dtype)
    f = fd.BuiltinF(family, N, dtype=dtype)
    lazy = getattr(f, "lazy_fn", None) is not None
    assert lazy or N < 3
    if lazy and path != "small":
        plan.set_lazy(f, fused=(path == "fused"))
    # the storing launch needs at least 3 cyclic colours on more than 3 columns; below that the plan keeps the hand-over path
    want_store = 1 if path in ("store", "fused") and N > 3 and C >= 3 else 0
    assert plan.info(fd.lib.INFO_LAZY_STORE) == want_store, (path, N, C)
    assert plan.info(fd.lib.INFO_SMALL_FUSED) == (1 if path == "small" else 0), path
    plan.enable_timing(2)
    plan.jacobian(f, torch.as_tensor(x, device="cuda"), _tridiag_outs(J), relstep=rel, absstep=ab, dir=dir)
    launches = plan.timings()["eps"]["launches"]
    plan.enable_timing(0)
    # the fused step has no step-size stage of its own; more than kRegColors = 8 colours always take the per-colour lists and
    # k_eps_finalize (launch_eps_t: the choice is C alone)
    assert launches == (0 if path == "fused" else 1), (path, C, launches)
    assert plan.info(fd.lib.INFO_NCOLORS) == C
    _check(plan, _tridiag_outs(J), _tridiag_layout(kind, N, c0), x, c0, C, fdtype, rel, ab, dir, dtype, X.fixture(family, N),
           defined_order=C <= 8 and path != "small")


SIZES = [1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048 * 64 * 3 + 1000]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tridiag_store_wave_sizes_and_colourings(monkeypatch, N, dtype):
    for i, (C, shift) in enumerate([(N, 0)] if N < 3 else [(3, 0), (5, 2), (8, 7)]):
        if C > N:
            continue
        fdtype = ("forward", "central")[i % 2]
        _run_tridiag(monkeypatch, N, C, shift, ("csc", "banded", "tridiagonal")[(i + N) % 3], dtype, fdtype, "ordinary",
                     dir=-1.0 if i == 2 else 1.0, path="store")


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("case", CASES64)
@pytest.mark.parametrize("path", ["store", "fused", "handover"])
def test_tridiag_float64_operands(monkeypatch, fdtype, case, path):
    N = 70_001 if path != "fused" else 40_003
    for kind in ("csc", "banded", "tridiagonal"):
        _run_tridiag(monkeypatch, N, 3 if kind != "banded" else 4, 1, kind, np.float64, fdtype, case,
                     dir=-1.0 if (fdtype == "forward" and kind == "banded") else 1.0, path=path)


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("case", CASES32)
@pytest.mark.parametrize("path", ["store", "fused"])
def test_tridiag_float32_operands(monkeypatch, fdtype, case, path):
    for kind in ("csc", "banded", "tridiagonal"):
        _run_tridiag(monkeypatch, 50_001, 3, 0, kind, np.float32, fdtype, case, path=path)


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("case", ["ordinary", "num_2p800", "huge_range", "tiny_1e-200", "subnormal", "nan_inf"])
@pytest.mark.parametrize("C", [9, 13])
def test_tridiag_many_colours_operands(monkeypatch, fdtype, case, C):
    # more colours than the reduction keeps in registers (kRegColors = 8): per-colour column lists and k_eps_finalize, whose
    # scaled rescan walks the colour's list
    _run_tridiag(monkeypatch, 70_001, C, 4, "csc", np.float64, fdtype, case, path="store")


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("case", ["ordinary", "num_2p800", "huge_range", "tiny_1e-200", "subnormal", "nan_inf"])
@pytest.mark.parametrize("N,C", [(3000, 3), (16_000, 8)])
def test_tridiag_small_problem_launch_operands(monkeypatch, fdtype, case, N, C):
    # the single-workgroup step-size launch of small problems (k_eps_perturb_small) and its scaled rescan
    _run_tridiag(monkeypatch, N, C, 1, "csc", np.float64, fdtype, case, path="small")


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("C", [3, 9])
@pytest.mark.parametrize("case", ["ordinary", "huge", "tiny"])
def test_complex_valued_x_step_sizes(monkeypatch, fdtype, C, case):
    # complex-valued x: the masked norm runs over |x_j|^2 = re^2 + im^2 (the (re, im) pair branch of every reduction and rescan).
    # The step sizes against the scaled norm evaluated on the host (4 ulps; the plain sum's order differs from the pair order), and
    # the Jacobian of the linear tridiagonal fixture finite
    monkeypatch.setenv("FDJAC_SMALL", "0")
    N = 40_000
    rng = np.random.default_rng(C)
    xh = (rng.random(N) + 0.5) + 1j * (rng.random(N) - 0.5)
    colors = P.cyclic_colors(N, C)
    if case == "huge":
        xh[colors == 1] *= 1e200
    elif case == "tiny":
        xh[colors == 2] *= 1e-200
    ab = 0.0 if case == "tiny" else None
    colptr, rowval = P.tridiag_csc(N)
    J = fd.SparseMatrixCSC(N, N, colptr, rowval, torch.full((rowval.size,), complex(float("nan"), float("nan")), dtype=torch.complex128,
                                                              device="cuda"))
    plan = fd.make_plan(J, J, colors, fdtype, complex_x=True)
    f = fd.BuiltinF("tridiag", N)
    plan.enable_timing(2)
    plan.jacobian(f, torch.as_tensor(xh, device="cuda"), [J.nzval], absstep=ab)
    launches = plan.timings()["eps"]["launches"]
    plan.enable_timing(0)
    assert launches == 1 and plan.info(fd.lib.INFO_NCOLORS) == C, (C, launches)
    got = plan.epsilons()
    rel = X.default_relstep(fdtype)
    for c in range(C):
        v = xh[colors == c + 1]
        with np.errstate(over="ignore"):
            t = float(np.sum(v.real ** 2 + v.imag ** 2))
        k = X.rescale_exp(t, rel, rel if ab is None else ab)
        y = v * 2.0 ** k
        nrm = np.sqrt(np.sum(y.real ** 2 + y.imag ** 2)) * 2.0 ** -k
        want = X.jl_max(rel * np.sqrt(nrm), rel if ab is None else ab)
        if (case, c) in (("huge", 0), ("tiny", 1)):
            assert k != 0, (case, c)                     # the case reaches the scaled rescan
        assert _ulps(np.array([got[c]]), np.array([want]))[0] <= 4, (case, c, got[c], want)
    assert torch.isfinite(torch.view_as_real(J.nzval)).all()


def test_tridiag_above_the_fused_limit(monkeypatch):
    # 2^21 + 3 columns: the two-launch form (the fused step stops at 2^21), an overflowing colour and a NaN among them
    _run_tridiag(monkeypatch, 2 ** 21 + 3, 3, 0, "csc", np.float64, "central", "num_2p800", path="store")
    _run_tridiag(monkeypatch, 2 ** 21 + 3, 5, 1, "csc", np.float64, "forward", "nan_inf", path="store")


def _run_stencil5(monkeypatch, nx, ny, dtype, fdtype, case, family="lap5_nl", dir=1.0, want_store=1):
    monkeypatch.setenv("FDJAC_SMALL", "0")
    monkeypatch.setenv("FDJAC_LAZY_STORE", "1")
    N = nx * ny
    cp, rv = P.lap5_csc(nx, ny)
    colors = P.lap5_colors(nx, ny)
    C = int(colors.max())
    c0 = colors - 1
    x, rel, ab = _operands(case, N, C, dtype, nx * 31 + ny)
    t = torch.float64 if dtype == np.float64 else torch.float32
    J = fd.SparseMatrixCSC(N, N, cp, rv, torch.full((rv.size,), float("nan"), dtype=t, device="cuda"))
    plan = fd.make_plan(J, J, colors, fdtype, dtype=dtype)
    f = fd.BuiltinF(family, nx, ny, dtype=dtype)
    assert getattr(f, "lazy_fn", None) is not None
    plan.set_lazy(f)
    assert plan.info(fd.lib.INFO_LAZY_STORE) == want_store      # (grids of two rows keep the hand-over path)
    plan.jacobian(f, torch.as_tensor(x, device="cuda"), [J.nzval], relstep=rel, absstep=ab, dir=dir)
    _check(plan, [J.nzval], lambda D: [X.to_csc(D, c0, cp, rv)], x, c0, C, fdtype, rel, ab, dir, dtype, X.fixture(family, nx, ny))


@pytest.mark.parametrize("nx", [6, 254, 256, 258, 1028])
@pytest.mark.parametrize("ny", [2, 3, 5])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_stencil5_store_grids(monkeypatch, nx, ny, dtype):
    for i, fdtype in enumerate(("forward", "central")):
        _run_stencil5(monkeypatch, nx, ny, dtype, fdtype, "ordinary", family=("lap5", "lap5_nl")[i], dir=-1.0 if i == 0 else 1.0,
                      want_store=1 if ny >= 3 else 0)


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("dtype,case", [(np.float64, c) for c in CASES64] + [(np.float32, c) for c in CASES32])
def test_stencil5_store_operands(monkeypatch, fdtype, case, dtype):
    _run_stencil5(monkeypatch, 258, 40, dtype, fdtype, case)
