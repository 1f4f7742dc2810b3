"""The three solvers on systems whose coupling spans EVERY level of their elimination (tests/solve_model.py): family E, whose solution
is known bit for bit (the assertion is equality with the int64 closed form), and family S, slow two-sided decay, against an
extended-precision refined reference with the tolerance 16 max(E_lapack, eps ||y||) (solve_model.s_tolerance).  The inputs of
test_gpu_solve.py / test_gpu_bandsolve.py / test_gpu_blocksolve.py decay within a few rows: everything above the first levels is
invisible to them; tests/test_solve_model_cpu.py proves that here a wrong coupling at any level (any rank's spike tips) fails.

Every solve is repeated on the same solver after a solve of the other family (stale pool / level state): the same bits; b is
untouched; y is NaN-filled before each call.  Each family-S check prints `ACCURACY <case> err E_lapack ratio`: the ratios of
profiles/solver_accuracy.md."""
import functools
import hashlib

import numpy as np
import pytest

import finitediff_jl_amd as fd
import solve_model as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = np.finfo(np.float64).eps
S_SHIFTS = [(1.0, -0.5), (0.0, 1.0), (0.0, -2.0)]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _nan(n, like):
    return torch.full((n,), float("nan"), dtype=like.dtype, device="cuda")


_REF = {}          # the last few refined references (a case's layouts run one after the other)


def _system_key(s):
    """What identifies a system: its shape, shift, element type and a digest of its right-hand side and diagonal."""
    h = hashlib.sha1(s.b.tobytes())
    h.update(s.A[0].tobytes())
    return (s.kind, s.N, s.alpha, s.beta, s.b.dtype.name, tuple(sorted(s.A)), h.hexdigest())


def _check_S(got, s, label, dtype=np.float64, factor=16.0):
    key = _system_key(s)
    if key not in _REF:
        while len(_REF) >= 2:
            _REF.pop(next(iter(_REF)))
        _REF[key] = M.refined_reference(s)
    yref, E = _REF[key]
    nrm = float(np.max(np.abs(yref)))
    err = float(np.max(np.abs(got.astype(np.longdouble) - yref)))
    tol = M.s_tolerance(yref, E, dtype, factor)
    print("ACCURACY %s err=%.3e E_lapack=%.3e ratio=%.2f of_tol=%.3f" % (label, err, E, err / max(E, EPS * nrm), err / tol))
    assert not np.isnan(got).any(), label
    assert err <= tol, (label, err, tol, E)


def _check_E(y, s, label):
    want = torch.as_tensor(s.y.astype(np.float64)).to(y.dtype)
    assert torch.equal(y.cpu(), want), (label, int((y.cpu() != want).sum()))


# ------------------------------------------------------------------------------------------------------------ tridiagonal
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


def _tri_J(s, layout):
    dl, d, du = s.J
    if layout == "diagonals":
        return fd.Tridiagonal(_dev(dl), _dev(d), _dev(du))
    return [_dev(_csc_nzval(dl, d, du))]


def _solve(solver, J, b, alpha, beta):
    keep = b.clone()
    y = _nan(b.numel(), b)
    solver.solve(J, b, y, alpha, beta)
    assert torch.equal(b, keep)
    return y


def _two_families(solver, sysE, JE, sysS, JS, label, dtype=np.float64, check_s=True):
    """E, S, E again, S again on ONE solver: E equals the closed form, S meets its tolerance, the repeats have the same bits."""
    bE, bS = _dev(sysE.b), _dev(sysS.b)
    yE = _solve(solver, JE, bE, sysE.alpha, sysE.beta)
    assert solver.status() == 0
    _check_E(yE, sysE, label)
    yS = _solve(solver, JS, bS, sysS.alpha, sysS.beta)
    assert solver.status() == 0
    assert not bool(torch.isnan(yS).any())
    if check_s:
        _check_S(yS.cpu().numpy(), sysS, label, dtype)
    assert torch.equal(_solve(solver, JE, bE, sysE.alpha, sysE.beta), yE)
    assert torch.equal(_solve(solver, JS, bS, sysS.alpha, sysS.beta), yS)
    return yE, yS


@functools.lru_cache(maxsize=2)
def _tri_pair(N, kind="segmented"):
    k = M.TRI_E_N.index(N) if N in M.TRI_E_N else N
    sysE = M.e_tridiag(N, 11 + N, kind, M.E_SHIFTS[k % 4])
    sysS = M.s_tridiag(N, M.tri_default_lam(N), 13 + N, shift=S_SHIFTS[k % 3])
    return sysE, sysS, N <= 3 * 10 ** 6 + 1       # family S is CHECKED up to 3 * 10^6 + 1 (the refined reference); beyond, it is the other family's solve


@pytest.mark.parametrize("N", M.TRI_E_N)
@pytest.mark.parametrize("layout", ["diagonals", "csc"])
def test_tridiagonal_whole_both_families(layout, N):
    sysE, sysS, check_s = _tri_pair(N)
    solver = fd.TridiagSolver(N, layout)
    _two_families(solver, sysE, _tri_J(sysE, layout), sysS, _tri_J(sysS, layout), "tri N=%d lam=%g @%s" % (N, sysS.meta["lam"], layout),
                  check_s=check_s)


@pytest.mark.parametrize("kind", ["lower", "upper"])
@pytest.mark.parametrize("N", M.TRI_CHAIN_N)
def test_tridiagonal_single_chain(kind, N):
    # one chain through the whole system: a prefix (suffix) sum across every tile, level and the top
    sysS = M.s_tridiag(N, M.tri_default_lam(N), 19 + N)
    for layout in ("diagonals", "csc"):
        solver = fd.TridiagSolver(N, layout)
        JS, bS = _tri_J(sysS, layout), _dev(sysS.b)
        for q, shift in enumerate(M.E_SHIFTS):
            s = M.e_tridiag(N, 17 + q, kind, shift)
            J, b = _tri_J(s, layout), _dev(s.b)
            y = _solve(solver, J, b, s.alpha, s.beta)
            _check_E(y, s, (kind, N, shift, layout))
            yS = _solve(solver, JS, bS, sysS.alpha, sysS.beta)               # the other family in between
            assert solver.status() == 0 and not bool(torch.isnan(yS).any())
            assert torch.equal(_solve(solver, J, b, s.alpha, s.beta), y)


def test_tridiagonal_slowest_decay():
    N, lam = 3 * 10 ** 6 + 1, 3.0e5
    s = M.s_tridiag(N, lam, 29)
    sysE = M.e_tridiag(N, 23, "segmented", (2.0, -1.0))
    for layout in ("diagonals", "csc"):
        solver = fd.TridiagSolver(N, layout)
        _two_families(solver, sysE, _tri_J(sysE, layout), s, _tri_J(s, layout), "tri N=%d lam=%g @%s" % (N, lam, layout))


@pytest.mark.parametrize("layout", ["diagonals", "csc"])
@pytest.mark.parametrize("N", M.TRI_SCHEDULE_N)
def test_tridiagonal_schedules_agree(layout, N, monkeypatch):
    # one level per launch (-1), two levels per launch from level 0 / from level 2: the same bits on family E, the tolerance on S
    sysE = M.e_tridiag(N, 31 + N, "segmented", M.E_SHIFTS[N % 4])
    sysS = M.s_tridiag(N, M.tri_default_lam(N), 37 + N)
    solver = fd.TridiagSolver(N, layout)
    JE, JS = _tri_J(sysE, layout), _tri_J(sysS, layout)
    ys = []
    for sched in ("-1", "0", "2"):
        monkeypatch.setenv("FDJAC_SOLVE_TWO_LEVEL", sched)
        yE, yS = _two_families(solver, sysE, JE, sysS, JS, "tri N=%d lam=%g schedule=%s @%s" % (N, sysS.meta["lam"], sched, layout))
        ys.append(yE)
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def test_tridiagonal_float32_solver():
    N = M.TRI_F32
    f32 = np.float32
    sysE = M.e_tridiag(N, 41, "segmented", (2.0, -1.0), dtype=f32)
    sysS = M.s_tridiag(N, M.tri_default_lam(N), 43, dtype=f32)
    solver = fd.TridiagSolver(N, "diagonals", dtype=f32)
    _two_families(solver, sysE, _tri_J(sysE, "diagonals"), sysS, _tri_J(sysS, "diagonals"), "tri f32 N=%d lam=%g" % (N, sysS.meta["lam"]),
                  dtype=f32)


def _rank_inputs(s, cuts, layout):
    """Per rank: its slice of J (as the column-window Jacobian plans leave it) and its rows of b."""
    N = s.N
    dl, d, du = s.J
    nz = _csc_nzval(dl, d, du)
    out = []
    for r in range(len(cuts) - 1):
        c0, c1 = int(cuts[r]), int(cuts[r + 1])
        if layout == "diagonals":
            J = fd.Tridiagonal(_dev(dl[c0:min(c1, N - 1)]), _dev(d[c0:c1]), _dev(du[max(c0 - 1, 0):c1 - 1]))
        else:
            e0 = 3 * c0 - 1 if c0 > 0 else 0
            e1 = 3 * c1 - 1 if c1 < N else 3 * N - 2
            J = [_dev(nz[e0:e1])]
        out.append((J, _dev(s.b[c0:c1])))
    return out


def _sharded(solvers, inputs, s, cuts):
    """interface on every rank -> the packets in one tensor -> finish on every rank, on the ranks' OWN solver objects."""
    W = len(cuts) - 1
    packets = torch.full((W, 8), float("nan"), dtype=torch.float64, device="cuda")
    for r, (J, bl) in enumerate(inputs):
        solvers[r].interface(J, bl, packets[r], s.alpha, s.beta)
    out = torch.full((s.N,), float("nan"), dtype=torch.float64, device="cuda")
    for r, (J, bl) in enumerate(inputs):
        keep = bl.clone()
        yl = _nan(bl.numel(), bl)
        solvers[r].finish(J, bl, packets, r, W, yl, s.alpha, s.beta)
        assert solvers[r].status() == 0 and torch.equal(bl, keep)
        out[cuts[r]:cuts[r + 1]] = yl
    return out


@pytest.mark.parametrize("N,cuts", M.TRI_SHARDED)
@pytest.mark.parametrize("layout", ["diagonals", "csc"])
def test_tridiagonal_sharded_both_families(layout, N, cuts):
    sysE = M.e_tridiag_crossing(N, cuts, 47 + N)
    lam = M.sharded_lam(cuts)                     # >= twice the largest rank: the interface matrix is far from the identity
    sysS = M.s_tridiag(N, lam, 53 + N)
    solvers = [fd.TridiagSolver(N, layout, rows=(int(cuts[r]), int(cuts[r + 1]))) for r in range(len(cuts) - 1)]
    inE, inS = _rank_inputs(sysE, cuts, layout), _rank_inputs(sysS, cuts, layout)
    y = _sharded(solvers, inE, sysE, cuts)
    _check_E(y, sysE, ("sharded", N, cuts, layout))
    whole = _solve(fd.TridiagSolver(N, layout), _tri_J(sysE, layout), _dev(sysE.b), sysE.alpha, sysE.beta)
    assert torch.equal(y, whole)
    yS = _sharded(solvers, inS, sysS, cuts)      # the other family through the SAME per-rank solvers
    _check_S(yS.cpu().numpy(), sysS, "tri sharded N=%d W=%d lam=%g @%s" % (N, len(cuts) - 1, lam, layout))
    assert torch.equal(_sharded(solvers, inE, sysE, cuts), y)
    assert torch.equal(_sharded(solvers, inS, sysS, cuts), yS)


# ------------------------------------------------------------------------------------------------------------ banded
def _band_vals(data, N, l, u, layout):
    if layout == "banded":
        return np.ascontiguousarray(data.T.reshape(-1))
    k = np.arange(l + u + 1)[None, :]
    i = np.arange(N)[:, None] - u + k                  # row of slot k in column j
    return np.ascontiguousarray(data.T[(i >= 0) & (i < N)])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N,l,u", M.BAND_SHAPES)
@pytest.mark.parametrize("layout", ["banded", "csc"])
def test_banded_both_families(dtype, layout, N, l, u):
    solver = fd.BandedSolver(N, l, u, layout=layout, dtype=dtype)
    q = M.BAND_SHAPES.index((N, l, u))
    sysS, sysEs = M.gpu_band_systems(N, l, u, dtype, s_shift=None if dtype == np.float32 else S_SHIFTS[q % 3])
    JS = _dev(_band_vals(sysS.J, N, l, u, layout))
    for sysE in sysEs:
        JE = _dev(_band_vals(sysE.J, N, l, u, layout))
        _two_families(solver, sysE, JE, sysS, JS, "band %s N=%d (l,u)=(%d,%d) lam=%g" % (np.dtype(dtype).name, N, l, u, sysS.meta["lam"]) + " @" + layout,
                      dtype)


# ------------------------------------------------------------------------------------------------------------ block tridiagonal
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nb,bs", M.BLOCK_SHAPES)
def test_block_tridiagonal_both_families(dtype, nb, bs):
    solver = fd.BlockTridiagSolver(nb, bs, dtype=dtype)
    sysS, sysEs = M.gpu_block_systems(nb, bs, dtype)
    JS = _dev(sysS.J)
    for sysE in sysEs:
        _two_families(solver, sysE, _dev(sysE.J), sysS, JS, "block %s nb=%d b=%d lam=%g" % (np.dtype(dtype).name, nb, bs, sysS.meta["lam"]), dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nb,bs", M.BLOCK_DENSE_SHAPES)
def test_block_tridiagonal_dense_blocks_under_the_trust_policy(dtype, nb, bs):
    # A = T_delta (x) G, G dense SPD with condition < 4: not row dominant.  Refused by default (all NaN, status bit 0); with
    # set_policy(True) the elimination's result, flag still raised -- and here its accuracy is checked
    q = M.BLOCK_DENSE_SHAPES.index((nb, bs))
    s = M.s_block_dense(nb, bs, M.block_lam(nb), 73 + q, dtype)
    sysE = M.e_block(nb, bs, 79 + q, True, (0.0, 1.0), dtype)
    solver = fd.BlockTridiagSolver(nb, bs, dtype=dtype)
    J, b = _dev(s.J), _dev(s.b)
    y = _solve(solver, J, b, s.alpha, s.beta)
    assert solver.status() & 1 and bool(torch.isnan(y).all())
    solver.set_policy(True)
    y = _solve(solver, J, b, s.alpha, s.beta)
    assert solver.status() & 1
    _check_S(y.cpu().numpy(), s, "block dense %s nb=%d b=%d lam=%g condG=%.2f" % (np.dtype(dtype).name, nb, bs, s.meta["lam"], s.meta["condG"]), dtype)
    yE = _solve(solver, _dev(sysE.J), _dev(sysE.b), sysE.alpha, sysE.beta)            # the other family in between
    assert solver.status() == 0
    _check_E(yE, sysE, ("block E after dense", nb, bs))
    assert torch.equal(_solve(solver, J, b, s.alpha, s.beta), y)
    solver.set_policy(False)
