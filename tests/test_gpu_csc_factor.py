"""The sparse consumer's factorisation and its application as operations of their own (fd_csc_solver_factor_async, _apply_async,
_factor_status; csrc/fdjac_cscsolve.hip): the factor's BITS against those a solve with the same arguments leaves and against the
models (tests/csc_block_model.py, tests/csc_ilu_model.py), the apply's bits against the models over the block edges, the Float32 build
(Float32 nzval, Float64 vectors), the status bit, the generation rule, and that a solve behind a factor is the solve it was."""
import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as M
import csc_block_model as BM
import csc_ilu_model as IM
import jfnk_pc_model as PM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CANARY = 7.25
KINDS = (("jacobi",), ("block", 2), ("block", 5), ("block", 32), ("ilu", 2), ("ilu", 64), ("ilu", 1024))
NAMES = ("1", "2", "33", "1023", "1025", "2049", "lap5")          # tridiagonal sizes; lap5 on a 7 x 9 grid

_systems = {}


def system(name):
    """(colptr, rowval, N, nz, x, gamma, RowLists): values and x in [-1, 1], A = I - gamma J with gamma * max ||row of J||_1 = 0.9."""
    if name not in _systems:
        colptr, rowval, N = M.lap5_pattern(7, 9) if name == "lap5" else M.tridiag_pattern(int(name))
        rng = np.random.default_rng(4000 + N)
        nz = rng.uniform(-1.0, 1.0, rowval.size)
        x = rng.uniform(-1.0, 1.0, N)
        rows = np.zeros(N)
        np.add.at(rows, rowval, np.abs(nz))
        _systems[name] = (colptr, rowval, N, nz, x, float(0.9 / rows.max()), M.RowLists(colptr, rowval, N))
    return _systems[name]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _solver(name, kind, dtype=np.float64):
    colptr, rowval, N = system(name)[:3]
    s = fd.CscSolver((colptr, rowval, N), dtype=dtype, idx_base=0)
    if kind[0] == "jacobi":
        s.set_preconditioner("jacobi")
    elif kind[0] == "block":
        s.set_preconditioner("block_jacobi", kind[1])
    else:
        s.set_block_ilu(kind[1])
    return s


def _factors(s, kind):
    """The factorisation's arrays as numpy, by the diagnostic accessors (none for the diagonal)."""
    if kind[0] == "block":
        return [s.block_inverses().cpu().numpy()]
    if kind[0] == "ilu":
        lu, u, _bs = s.ilu_factors()
        return [lu.cpu().numpy(), u.cpu().numpy()]
    return []


def _apply(s, x):
    N = x.size
    buf = torch.full((N + 2,), CANARY, dtype=torch.float64, device="cuda")
    s.apply_preconditioner(_dev(x), buf[1:1 + N])
    h = buf.cpu().numpy()
    assert h[0] == CANARY and h[-1] == CANARY
    return h[1:1 + N]


def _solve(s, nz, b, gamma, dtype=np.float64):
    s.set_options(1e-10 if dtype == np.float64 else 1e-6, 40)
    s.set_policy(True)
    y = torch.full((b.size,), 7.0, dtype=_dev(b.astype(dtype)).dtype, device="cuda")
    s.solve(_dev(nz.astype(dtype)), _dev(b.astype(dtype)), y, 1.0, -gamma)
    return y.cpu().numpy(), s.status()


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: "".join(map(str, k)))
@pytest.mark.parametrize("name", NAMES)
def test_factor_and_apply_equal_a_solves_bits_and_the_models(name, kind):
    colptr, rowval, N, nz, x, gamma, rl = system(name)
    s = _solver(name, kind)
    s.factor(_dev(nz), 1.0, -gamma)
    assert s.factor_status() == {"flags": 0}
    got = _factors(s, kind)
    z = _apply(s, x)
    # the models: the factorisation's arrays, then out = M^-1 x
    if kind[0] == "block":
        planes, bad = BM.block_inverses(colptr, rowval, N, 1.0, -gamma, nz, kind[1])
        assert not bad and _same(got[0], planes)
    elif kind[0] == "ilu":
        lu, u, bad = IM.factor(IM.Schedule(rl, kind[1]), 1.0, -gamma, nz)
        assert not bad and _same(got[0], lu) and _same(got[1], u)
    apply, bad = PM.factorisation(rl, 1.0, -gamma, nz, kind)
    assert not bad and _same(z, apply(x))
    assert _same(_apply(s, x), z)                              # the factorisation stands: applied again, the same bits
    # a solve with the same arguments leaves the same factorisation
    t = _solver(name, kind)
    _solve(t, nz, x, gamma)
    for a, b in zip(got, _factors(t, kind)):
        assert _same(a, b)


def test_the_float32_build_factors_float32_values_and_applies_to_doubles():
    name, kind = "1025", ("block", 5)
    colptr, rowval, N, nz, x, gamma, rl = system(name)
    nz32 = nz.astype(np.float32)
    for kind in (("block", 5), ("ilu", 64), ("jacobi",)):
        s = _solver(name, kind, np.float32)
        s.factor(_dev(nz32), 1.0, -gamma)
        apply, bad = PM.factorisation(rl, 1.0, -gamma, nz32.astype(np.float64), kind)
        z = _apply(s, x)                                       # x is NOT representable in Float32: the vectors are doubles
        assert not bad and s.factor_status() == {"flags": 0} and _same(z, apply(x)), kind
        with pytest.raises(TypeError):
            s.apply_preconditioner(_dev(x.astype(np.float32)), torch.empty(N, dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("kind", [("jacobi",), ("block", 2), ("ilu", 2)], ids=lambda k: "".join(map(str, k)))
def test_status_bit_1_for_a_block_with_two_equal_rows(kind):
    colptr, rowval, N, nz, x, gamma, rl = system("33")
    cols = np.repeat(np.arange(N), np.diff(colptr))
    nz = nz.copy()
    for r, c, a in ((0, 0, 2.0), (0, 1, 2.0), (1, 0, 2.0), (1, 1, 2.0)):          # block 0 of I - gamma J becomes [[2, 2], [2, 2]]
        q = np.nonzero((rowval == r) & (cols == c))[0][0]
        nz[q] = (a - (1.0 if r == c else 0.0)) / -gamma
    if kind[0] == "jacobi":
        nz[rl.diag[7]] = 1.0 / gamma                           # the diagonal alone sees no equal rows: a zero diagonal instead
    s = _solver("33", kind)
    s.factor(_dev(nz), 1.0, -gamma)
    assert s.factor_status() == {"flags": 2}
    assert PM.factorisation(rl, 1.0, -gamma, nz, kind)[1]
    s.factor(_dev(system("33")[3]), 1.0, -gamma)               # the word is the factorisation's: the next one clears it
    assert s.factor_status() == {"flags": 0}
    # ... and no solve does: a solve on ANOTHER factorisation's handle state leaves the factor's word alone
    s.factor(_dev(nz), 1.0, -gamma)
    _solve(s, system("33")[3], x, gamma)
    assert s.factor_status() == {"flags": 2} and s.status()["flags"] == 0


def test_errors_and_the_generation_rule():
    colptr, rowval, N, nz, x, gamma, rl = system("1025")
    s = _solver("1025", ("block", 5))
    xd = _dev(x)
    out = torch.empty_like(xd)
    with pytest.raises(fd.lib.FdError) as e:
        s.apply_preconditioner(xd, out)                        # before any factor
    assert e.value.code == 3
    with pytest.raises(fd.lib.FdError) as e:
        s.factor_status()
    assert e.value.code == 3
    s.factor(_dev(nz), 1.0, -gamma)
    with pytest.raises(fd.lib.FdError) as e:
        s.apply_preconditioner(xd, xd)                         # out == x
    assert e.value.code == 1
    with pytest.raises(ValueError):
        s.apply_preconditioner(xd[:-1], out[:-1])
    s.apply_preconditioner(xd, out)
    want = out.clone()
    _solve(s, nz, x, gamma)                                    # a later solve: the buffers are its own
    with pytest.raises(fd.lib.FdError) as e:
        s.apply_preconditioner(xd, out)
    assert e.value.code == 9 and "stale" in str(e.value)
    s.factor(_dev(nz), 1.0, -gamma)
    s.apply_preconditioner(xd, out)
    assert torch.equal(out, want)
    for setter in (lambda: s.set_preconditioner("block_jacobi", 5), lambda: s.set_preconditioner("jacobi"), lambda: s.set_block_ilu(64)):
        s.factor(_dev(nz), 1.0, -gamma)
        s.apply_preconditioner(xd, out)
        setter()                                               # a later setter, even one that selects what is selected
        with pytest.raises(fd.lib.FdError) as e:
            s.apply_preconditioner(xd, out)
        assert e.value.code == 9


@pytest.mark.parametrize("kind", [("jacobi",), ("block", 32), ("ilu", 64)], ids=lambda k: "".join(map(str, k)))
@pytest.mark.parametrize("method", ["bicgstab", "gmres"])
def test_a_solve_behind_a_factor_is_the_solve_it_was(kind, method):
    colptr, rowval, N, nz, x, gamma, rl = system("2049")
    a, b = _solver("2049", kind), _solver("2049", kind)
    for s in (a, b):
        s.set_method(method, 5)
    b.factor(_dev(nz * 0.5), 0.75, -0.5 * gamma)               # another matrix's factorisation in the buffers the solve reuses
    ya, sa = _solve(a, nz, x, gamma)
    yb, sb = _solve(b, nz, x, gamma)
    assert sa == sb and sa["flags"] == 0 and _same(ya, yb)
