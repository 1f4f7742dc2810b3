"""The trust-region consumer on the device (csrc/fdjac_csctr.hip): the product and the Steihaug-Toint step BIT FOR BIT against the numpy
model (tests/csc_tr_model.py) -- y, r_out, the exit kind, the flags, the iteration count and the four status scalars, for every case of
tests/test_csctr_model_cpu.py and both norms --, the derived bounds of that file on the device's own y, the failure paths, the arguments,
the path end to end behind a Hessian and a gradient the library has just stored, and the square solver beside it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_solve_model as SM
import csc_tr_model as TM
import test_csctr_model_cpu as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, MAXIT, INF = H.RTOL, H.MAXIT, H.INF
NORMS = {0: "I", 1: "diag"}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _same_bits(got, want):
    return got.dtype == want.dtype and np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


def _tr(colptr, rowval, N, idx=np.int64, base=0, device=False):
    cp, rv = (colptr + base).astype(idx), (rowval + base).astype(idx)
    if device:
        cp, rv = _dev(cp), _dev(rv)
    return fd.CscTrustRegion((cp, rv, N), idx_base=base)


def _device_step(s, nz, g, radius, lam, kind, rtol=RTOL, maxit=MAXIT, keep=False, with_r=True):
    s.set_options(rtol, maxit)
    s.set_policy(keep)
    y = torch.full((s.N,), 7.0, dtype=torch.float64, device="cuda")
    r = torch.full((s.N,), 7.0, dtype=torch.float64, device="cuda") if with_r else None
    s.step(_dev(nz), _dev(g), y, radius, lam, NORMS[kind], r_out=r)
    return y.cpu().numpy(), (r.cpu().numpy() if with_r else None), s.status()


_consumers = {}


def consumer(name):
    """One consumer per named case, shared by the tests below: every later step on it is also a test of its reuse."""
    if name not in _consumers:
        colptr, rowval, nz, N, g, rl = H.case(name)
        _consumers[name] = _tr(colptr, rowval, N)
    return _consumers[name]


@pytest.mark.parametrize("name", ["spd", "spd_long", "indef", "tiny"])
def test_product_is_bit_identical_to_the_model(name):
    pats = [TM.tiny_case(n) for n in (1, 2, 3)] if name == "tiny" else [H.case(name)[:4]]
    rng = np.random.default_rng(21)
    for colptr, rowval, nz, N in pats:
        rl = TM.RowLists(colptr, rowval, N)
        s = _tr(colptr, rowval, N)
        Hd = _dev(nz)
        for lam in (0.0, 0.7):
            v = rng.uniform(-1, 1, N)
            want = TM.matvec(rl, lam, nz, v)
            vd = _dev(v)
            for _ in range(2):
                y = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
                s.matvec(Hd, vd, y, lam)
                assert _same_bits(y.cpu().numpy(), want), (name, N, lam)


@pytest.mark.parametrize("name,lam,kind,radius", H.ALL_STEPS)
def test_step_is_bit_identical_to_the_model_and_meets_the_derived_bounds(name, lam, kind, radius):
    colptr, rowval, nz, N, g, rl = H.case(name)
    want_y, want_r, wst, _trace = H.model_step(name, lam, kind, radius)
    assert wst["flags"] == 0
    delta = H.radius_of(name, lam, kind, radius)
    s = consumer(name)
    for _ in range(2):                                   # twice on one consumer: the ticket, the `done` word and the exit word are reused
        y, r, st = _device_step(s, nz, g, delta, lam, kind)
        print("%s lam %g kind %d radius %s: %s (model %s)" % (name, lam, kind, radius, st, wst))
        assert TM.same_status(st, wst)
        assert _same_bits(y, want_y) and _same_bits(r, want_r)
    if wst["exit"] == 0:
        if H.sp is not None:
            err, bound, rel = H.derived_bound(name, lam, y)
            print("    error %.3e bound %.3e = %.3e ||y_ref||" % (err, bound, rel))
            assert rel <= 1e-6
            assert err <= bound
        H.check_pred(name, lam, kind, y, r, st)
    else:
        H.check_boundary_step(name, lam, kind, radius, y, r, st)
    y2, _none, st2 = _device_step(s, nz, g, delta, lam, kind, with_r=False)      # without r_out
    assert _same_bits(y2, want_y) and TM.same_status(st2, wst)


def test_step_is_bit_identical_under_batch_sizes_1_and_8():
    """Every step case, FDJAC_CSC_BATCH in {1, 8}: in a child process of its own (tests/csctr_switch_child.py) with
    FDJAC_TEST_SWITCHES=1.  The interior runs of 16 and 22 iterations end in the middle of a batch of 8, the boundary exits in the
    first one: the kernels enqueued behind the exit leave on `done`."""
    env = dict(os.environ, FDJAC_TEST_SWITCHES="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "csctr_switch_child.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout and out.stdout.count(": ok ") == 2 * len(H.ALL_STEPS) and "MISMATCH" not in out.stdout


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("idx", [np.int32, np.int64])
def test_index_types_bases_and_device_patterns(idx, base, device):
    name, lam, kind, radius = "spd_long", 0.25, 1, "inf"
    colptr, rowval, nz, N, g, rl = H.case(name)
    want_y, want_r, wst, _trace = H.model_step(name, lam, kind, radius)
    s = _tr(colptr, rowval, N, idx=idx, base=base, device=device)
    y, r, st = _device_step(s, nz, g, INF, lam, kind)
    assert TM.same_status(st, wst) and _same_bits(y, want_y) and _same_bits(r, want_r)


def test_a_bad_pattern_and_every_bad_argument_is_an_error_and_launches_nothing():
    colptr, rowval, nz, N, g, rl = H.case("spd")
    k = 7
    bad_row = rowval.copy(); bad_row[colptr[k + 1] - 1] = N
    unsorted = rowval.copy(); unsorted[[colptr[k], colptr[k] + 1]] = unsorted[[colptr[k] + 1, colptr[k]]]
    bad_ptr = colptr.copy(); bad_ptr[k] = bad_ptr[k + 1] + 1
    for cp, rv in ((colptr, bad_row), (colptr, unsorted), (bad_ptr, rowval)):
        for device in (False, True):
            with pytest.raises(fd.lib.FdError) as e:
                _tr(cp, rv, N, device=device)
            assert e.value.code == 2                   # FD_ERR_SHAPE
    with pytest.raises(ValueError):                    # colptr against N + 1
        _tr(colptr[:-1], rowval, N)
    with pytest.raises(ValueError):                    # a rectangular pattern
        fd.CscTrustRegion(fd.SparseMatrixCSC(N + 1, N, colptr + 1, rowval + 1, None))
    s = consumer("spd")
    yd, rd = (torch.full((N,), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    gd, nzd = _dev(g), _dev(nz)
    bad = [(-1e-3, 1.0, 0), (float("nan"), 1.0, 1), (INF, 1.0, 0), (0.0, 0.0, 0), (0.0, -1.0, 1), (0.0, float("nan"), 0), (0.0, 1.0, 2), (0.0, 1.0, -1)]
    for lam, radius, kind in bad:
        with pytest.raises(fd.lib.FdError) as e:
            s.step(nzd, gd, yd, radius, lam, kind, r_out=rd)
        assert e.value.code == 1, (lam, radius, kind)  # FD_ERR_ARG
    for lam in (-1.0, float("nan"), INF):
        with pytest.raises(fd.lib.FdError) as e:
            s.matvec(nzd, gd, yd, lam)
        assert e.value.code == 1
    with pytest.raises(fd.lib.FdError) as e:           # y must not be v
        s.matvec(nzd, gd, gd, 0.0)
    assert e.value.code == 1
    L = s.ctx.L
    for args in ((None, gd.data_ptr(), yd.data_ptr()), (nzd.data_ptr(), None, yd.data_ptr()), (nzd.data_ptr(), gd.data_ptr(), None)):
        assert L.fd_csc_tr_step_async(s.handle, 0.0, 1.0, 0, args[0], args[1], args[2], None) == 1
    assert L.fd_csc_tr_step_async(None, 0.0, 1.0, 0, nzd.data_ptr(), gd.data_ptr(), yd.data_ptr(), None) == 1
    s.ctx.synchronize()
    assert torch.all(yd == 7.0) and torch.all(rd == 7.0)          # nothing was launched


def test_failure_paths_are_loud_and_equal_the_model():
    colptr, rowval, nz, N, g, rl = H.case("spd")
    s = consumer("spd")

    def both(lists, cons, vals, gg, radius, lam, kind, maxit=MAXIT, keep=False):
        wy, wr, wst = TM.step(lists, lam, radius, kind, vals, gg, RTOL, maxit, keep_unconverged=keep)
        y, r, st = _device_step(cons, vals, gg, radius, lam, kind, maxit=maxit, keep=keep)
        assert TM.same_status(st, wst), (st, wst)
        assert _same_bits(y, wy) and _same_bits(r, wr)
        return y, r, st

    # the iterations run out
    y, r, st = both(rl, s, nz, g, INF, 0.0, 0, maxit=3)
    assert st["flags"] == 1 and st["iterations"] == 3 and np.all(np.isnan(y)) and np.all(np.isnan(r))
    y, r, st = both(rl, s, nz, g, INF, 0.0, 0, maxit=3, keep=True)
    assert st["flags"] == 1 and np.all(np.isfinite(y)) and np.all(np.isfinite(r))
    # a zero diagonal with the diagonal norm: the value, and the entry that is not stored
    nz0 = nz.copy(); nz0[rl.diag[17]] = 0.0
    cp1, rv1, nz1 = H.without_diagonal_entry(colptr, rowval, nz, 17, rl)
    rl1, s1 = TM.RowLists(cp1, rv1, N), _tr(cp1, rv1, N)
    for lists, cons, vals in ((rl, s, nz0), (rl1, s1, nz1)):
        y, r, st = both(lists, cons, vals, g, INF, 0.0, 1)
        assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
        y, r, st = both(lists, cons, vals, g, INF, 0.0, 1, keep=True)
        assert st["flags"] == 2 and not y.any() and _same_bits(r, g)
        for lam, kind in ((0.5, 1), (0.0, 0)):           # the same consumer is clean again
            y, r, st = both(lists, cons, vals, g, 1.0, lam, kind)
            assert st["flags"] == 0 and st["exit"] == 1
    # negative curvature and no boundary
    ic, ir, inz, iN, ig, il = H.case("indef")
    si = consumer("indef")
    for kind in (0, 1):
        y, r, st = both(il, si, inz, ig, INF, 0.0, kind)
        assert st["flags"] == 2 and st["exit"] == 3 and np.all(np.isnan(y))
        y, r, st = both(il, si, inz, ig, INF, 0.0, kind, keep=True)
        assert st["flags"] == 2 and st["exit"] == 3 and np.all(np.isfinite(y)) and st["step_norm"] > 0
        y, r, st = both(il, si, inz, ig, 1e200, 0.0, kind)
        assert st["flags"] == 2 and st["exit"] == 3
    # a NaN in H
    nzn = nz.copy(); nzn[5] = np.nan
    for kind in (0, 1):
        y, r, st = both(rl, s, nzn, g, INF, 0.0, kind)
        assert st["flags"] == 2 and np.all(np.isnan(y)) and np.all(np.isnan(r))
        y, r, st = both(rl, s, nzn, g, INF, 0.0, kind, keep=True)
        assert st["flags"] == 2
    # g = 0: y = 0, no iteration; and the consumer is clean again afterwards
    y, r, st = both(rl, s, nz, np.zeros(N), 1.0, 0.0, 1)
    assert st["flags"] == 0 and st["iterations"] == 0 and st["exit"] == 0 and not y.any() and not r.any()
    y, r, st = both(rl, s, nz, g, INF, 0.0, 1)
    assert st["flags"] == 0 and st["exit"] == 0


@pytest.mark.parametrize("N", [1, 2, 3])
def test_tiny_cases(N):
    colptr, rowval, nz, N = TM.tiny_case(N)
    rl = TM.RowLists(colptr, rowval, N)
    s = _tr(colptr, rowval, N)
    g = np.arange(1.0, N + 1)
    for vals, radius, kind in ((nz, INF, 0), (nz, INF, 1), (nz, 0.1, 1), (-nz, INF, 0), (-nz, 2.0, 0)):
        wy, wr, wst = TM.step(rl, 0.0, radius, kind, vals, g)
        y, r, st = _device_step(s, vals, g, radius, 0.0, kind)
        assert TM.same_status(st, wst) and _same_bits(y, wy) and _same_bits(r, wr), (N, radius, kind, st, wst)


CONCAVE_SRC = r"""
struct ConcaveChain {
    long long n;
    template <class P> __device__ real_t operator()(long long r, const P &X) const
    {
        const real_t b = X(r), a0 = X(r > 0 ? r - 1 : r), c0 = X(r + 1 < n ? r + 1 : r);
        const real_t a = r > 0 ? a0 : 0.0, c = r + 1 < n ? c0 : 0.0;
        const real_t d = (a - 2 * b) + c;
        return (b * b * b * b / 12 + (r % 3 == 0 ? -2.0 : 2.0) * b * b) + 0.1 * d * d;
    }
};
"""


def test_trust_region_step_on_a_hessian_and_gradient_the_library_stored():
    """phi_r = s_r 2 x_r^2 + x_r^4 / 12 + 0.1 (x_{r-1} - 2 x_r + x_{r+1})^2, s_r = -1 for r = 0 mod 3: H = diag(4 s + x^2) + 0.2 D^T D is
    indefinite (H_rr < 0 for r = 0 mod 3 and |x| <= 1/2: 4 s_r + x_r^2 + 1.2 <= -2.55).  Hessian, gradient and step are enqueued on one
    stream; nothing is read back in between."""
    n = 2000
    j = np.arange(n, dtype=np.int64)
    rows = np.stack([j - 1, j, j + 1], axis=1)
    has = (rows >= 0) & (rows < n)
    S = fd.SparseMatrixCSC(n, n, np.concatenate([[0], np.cumsum(has.sum(axis=1))]).astype(np.int64) + 1, rows[has].astype(np.int64) + 1, None)
    f = fd.ObjectiveF(CONCAVE_SRC, "ConcaveChain", n, n, params=np.array([n], np.int64).tobytes())
    x = _dev(0.5 * np.sin(np.arange(1, n + 1.0)))
    hc = fd.HessianCache(x, S, dest="csc")
    gc = fd.GradientCache(x, "central", S)
    Pm = hc.pattern()
    s = fd.CscTrustRegion(Pm)
    nzd = torch.full((Pm.rowval.size,), float("nan"), dtype=torch.float64, device="cuda")
    gd = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    radius = 1000.0
    out = {}
    for kind in (0, 1):
        y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        r = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        fd.finite_difference_hessian_b(nzd, f, x, hc)
        fd.finite_difference_gradient_b(gd, f, x, gc)
        s.step(nzd, gd, y, radius, 0.0, NORMS[kind], r_out=r)
        out[kind] = (y.cpu().numpy(), r.cpu().numpy(), s.status())
    vals, g = nzd.cpu().numpy(), gd.cpu().numpy()
    cp, rv = Pm.colptr - 1, Pm.rowval - 1
    rl = TM.RowLists(cp, rv, n)
    assert np.all(rl.diag >= 0) and np.all(vals[rl.diag][0::3] < -2.0)           # indefinite: e_r.H e_r < 0 < e_{r+1}.H e_{r+1}
    assert np.all(vals[rl.diag][1::3] > 2.0)
    cols = np.repeat(np.arange(n), np.diff(cp))
    for kind in (0, 1):
        y, r, st = out[kind]
        wy, wr, wst = TM.step(rl, 0.0, radius, kind, vals, g)
        print("end to end kind %d: %s" % (kind, st))
        assert st["flags"] == 0 and st["exit"] == 2 and TM.same_status(st, wst)
        assert _same_bits(y, wy) and _same_bits(r, wr)
        yl = y.astype(np.longdouble)
        Hy = np.zeros(n, dtype=np.longdouble)
        np.add.at(Hy, rv, vals.astype(np.longdouble) * yl[cols])
        q = (g.astype(np.longdouble) * yl).sum() + (yl * Hy).sum() / 2
        print("    q(y) = %.6e, pred = %.6e" % (float(q), st["pred"]))
        assert q < 0


def test_the_square_solver_is_untouched_by_a_trust_region_step_beside_it():
    colptr, rowval, nz, N, g, rl = H.case("spd_long")
    sq = fd.CscSolver((colptr, rowval, N), idx_base=0)
    sq.set_options(1e-12, 60)

    def square():
        y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        sq.solve(_dev(nz), _dev(g), y, 0.0, 1.0)
        return y.cpu().numpy(), sq.status()

    before, st_before = square()
    want, wst = SM.solve(SM.RowLists(colptr, rowval, N), 0.0, 1.0, nz, g, 1e-12, 60)
    assert st_before == wst and st_before["flags"] == 0 and _same_bits(before, want)
    s = consumer("spd_long")
    assert s.ctx is sq.ctx
    _, _, st = _device_step(s, nz, g, 1.0, 0.0, 1)
    assert st["flags"] == 0 and st["exit"] == 1
    after, st_after = square()
    assert st_after == st_before and _same_bits(after, before)


def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "csc_tr_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "csc_tr_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "status 0 exit 2" in out.stdout, out.stdout
