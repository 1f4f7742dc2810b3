"""The matrix-free consumer on the device (csrc/fdjac_jfnk.hip, fd_jfnk_*): every solve BIT FOR BIT against the numpy model
(tests/jfnk_model.py) on y, flags, iterations, estimate, ||b||, the last cycle's V and H and its length, over the covering set of
tests/jfnk_cases.py; the operator alone against torch's alpha z + beta q with q from the public fd_jvp_async; the ends of a solve, the
failures, the counts, a compiled functor against its built-in twin, and two solves of the sparse consumer's GMRES as a guard of the
shared host loop.

Accuracy: the device equals the model bit for bit, so the true residual of the device's y is the model's; the bound is 4 x the model's
worst value per family (tests/test_jfnk_model_cpu.py measures them; profiles/jfnk_accuracy.md has the table)."""
import os
import subprocess

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_gmres_model as G
import jfnk_cases as JK
import jfnk_model as JM
import test_jfnk_model_cpu as CPU

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CANARY = 7.25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count      # what fd_ctx holds: the grid of the large dot kernels


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _dev(a, off=0):
    """a on the device, `off` elements into a fresh allocation: off = 1 is misaligned to a pair; canaries on either side."""
    n = a.size
    buf = torch.full((n + 2 + off,), CANARY, dtype=torch.float64, device="cuda")
    buf[1 + off:1 + off + n] = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    return buf, buf[1 + off:1 + off + n]


def _canaries_ok(buf, off, n):
    h = buf.cpu().numpy()
    return np.all(h[:1 + off] == CANARY) and np.all(h[1 + off + n:] == CANARY)


def _f(case):
    return fd.BuiltinF(case["family"], *case["prm"])


def _solver(case, f, monkeypatch=None, restart=None, batch=None):
    if monkeypatch is not None:
        monkeypatch.setenv("FDJAC_SMALL", "0" if case["small_off"] else "1")
        if batch is not None:
            monkeypatch.setenv("FDJAC_CSC_BATCH", str(batch))
    s = fd.JfnkSolver(JK.size_of(case["family"], case["prm"]), case["fdtype"], case["restart"] if restart is None else restart)
    s.set_lazy(f if case["route"] != "plain" else None, quotient=case["route"] == "quot")
    return s


def _fx(f, xd):
    """f(x) on the device by one plain launch of the family's own launcher."""
    out = torch.empty_like(xd)
    n = xd.numel()
    rc = f.fn(f.fctx, out.data_ptr(), xd.data_ptr(), 1, n, n, 0, n, 0, f.ctx.stream)
    assert rc == 0
    return out


def _run(case, s, f, keep=True, maxit=None, rtol=None, b=None, d=None, x=None):
    """One device solve of the case: (y, status, V, H, len, counts before and after)."""
    _f0, x0, b0, d0 = JK.system(case["family"], case["prm"])
    x, b, d = (x0 if x is None else x), (b0 if b is None else b), (d0 if d is None else d)
    N = x.size
    _xb, xd = _dev(x, 1 - case["xoff"])            # (the canary takes one element: an odd offset is the aligned one)
    _bb, bd = _dev(b, 1 - case["boff"])
    _db, dd = _dev(d, 1 - case["doff"])
    assert (xd.data_ptr() % 16 == 0) == (not case["xoff"]) and (dd.data_ptr() % 16 == 0) == (not case["doff"])
    ybuf, yd = _dev(np.full(N, CANARY), 1)
    s.set_options(case["rtol"] if rtol is None else rtol, case["maxit"] if maxit is None else maxit)
    s.set_policy(keep)
    s.set_diagonal(dd if case["diag"] else None)
    fin = _fx(f, xd) if case["fin"] and case["fdtype"] == "forward" else None
    before = s.counts()
    s.solve(f, xd, bd, yd, 1.0, -JK.GAMMA, f_in=fin)
    st = s.status()
    V, H, k = s.basis()
    assert _canaries_ok(ybuf, 1, N)
    return yd.cpu().numpy(), st, V.cpu().numpy(), H.cpu().numpy(), k, before, s.counts()


def _compare(case, got, want, wst, tr):
    y, st, V, H, k, before, after = got
    print(case["id"], st, wst, "len", k, tr["len"])
    assert st == wst
    assert _same(y, want)
    assert k == tr["len"] and _same(V[:k], tr["V"][:k]) and _same(H[:k], tr["H"][:k])
    base = 1 if (case["fdtype"] == "forward" and not case["fin"]) else 0
    assert after[1] - before[1] == base and after[0] - before[0] >= tr["applications"]


def test_the_cases_cover():
    for n in JK.TILE_SIZES + JK.SWITCH_SIZES:
        assert any(JK.size_of(c["family"], c["prm"]) == n for c in JK.CASES), n
    assert {c["restart"] for c in JK.CASES} == set(JK.RESTARTS)
    assert {c["family"] for c in JK.CASES} == {"tridiag", "tridiag_nl", "lap5", "lap5_nl"}
    both = {False, True}
    for fam in ("tridiag", "tridiag_nl", "lap5", "lap5_nl"):          # every route on EACH family
        mine = [c for c in JK.CASES if c["family"] == fam]
        assert {c["fdtype"] for c in mine} == {"forward", "central"}, fam
        assert {bool(c["fin"]) for c in mine if c["fdtype"] == "forward"} == both, fam          # (the central arm never reads f_in)
        assert {c["route"] for c in mine} == {"plain", "lazy", "quot"}, fam
        for key in ("diag", "xoff", "boff"):
            assert {bool(c[key]) for c in mine} == both, (fam, key)
        assert {bool(c["doff"]) for c in mine if c["diag"]} == both, fam
        big = [c for c in mine if JK.size_of(c["family"], c["prm"]) > 16384]
        # above kSmallN: a caller's f_in through a lazy launcher (values, the quotient refused), and the opening kernel
        assert any(c["fin"] and c["fdtype"] == "forward" and c["route"] != "plain" for c in big), fam
        assert any(c["diag"] for c in big) and any(not c["diag"] for c in big), fam
    big = [c for c in JK.CASES if JK.size_of(c["family"], c["prm"]) > 16384]
    assert {(c["fdtype"], c["route"]) for c in big} == {(a, r) for a in ("forward", "central") for r in ("plain", "lazy", "quot")}
    odd = [c for c in big if JK.size_of(c["family"], c["prm"]) % 2 == 1]
    assert any(c["diag"] and c["doff"] for c in odd) and any(c["diag"] and not c["doff"] for c in odd)      # v_j off a pair at odd j, d on / off one
    assert any(not c["diag"] and not c["xoff"] for c in odd)                                               # the JVP's own dot alternates with j
    assert 60 <= len(JK.CASES) <= 90


@pytest.mark.parametrize("case", JK.CASES + JK.CONVERGENCE, ids=lambda c: c["id"])
def test_solve_equals_the_model_bit_for_bit(monkeypatch, num_cus, case):
    f = _f(case)
    s = _solver(case, f, monkeypatch)
    tr = {}
    want, wst = JK.model(case, num_cus, trace=tr)
    got = _run(case, s, f)
    _compare(case, got, want, wst, tr)
    again = _run(case, s, f)                      # the same bits on every call
    assert again[1] == got[1] and _same(again[0], got[0])
    if case in JK.CONVERGENCE:
        _f0, x, b, _d = JK.system(case["family"], case["prm"])
        res = JM.true_residual(case["family"], case["prm"], x, 1.0, -JK.GAMMA, b, got[0])
        print("true residual %.3e" % res, "bound %.3e" % (4 * CPU.MODEL_WORST[case["family"]]))
        assert wst["flags"] == 0 and res <= 4 * CPU.MODEL_WORST[case["family"]]


@pytest.mark.parametrize("case", JK.CASES, ids=lambda c: c["id"])
def test_apply_equals_torch_on_the_public_jvp(monkeypatch, case):
    """w = alpha z + beta q with q from fd_jvp_async(f_in = f(x)): no numpy model in this oracle."""
    f = _f(case)
    s = _solver(case, f, monkeypatch)
    _f0, x, _b, _d = JK.system(case["family"], case["prm"])
    N = x.size
    z = np.random.default_rng(N + 5).uniform(-1.0, 1.0, N)
    _xb, xd = _dev(x, 1 - case["xoff"])
    _zb, zd = _dev(z, 1 - case["boff"])
    wbuf, wd = _dev(np.full(N, CANARY), 1 - case["doff"])
    fx = _fx(f, xd)
    alpha, beta = 0.75, -JK.GAMMA
    before = s.counts()
    s.apply(f, xd, zd, wd, alpha, beta, f_in=fx if case["fin"] else None)
    after = s.counts()
    q = torch.empty(N, dtype=torch.float64, device="cuda")
    cache = fd.JVPCache(xd, case["fdtype"], lazy=case["route"] != "plain", quotient=False)
    fd.finite_difference_jvp_b(q, f, xd, zd, cache, f_in=fx, sync=False)
    want = alpha * zd + beta * q
    torch.cuda.synchronize()
    assert _same(wd.cpu().numpy(), want.cpu().numpy())
    assert _canaries_ok(wbuf, 1 - case["doff"], N)
    assert after[0] - before[0] == 1 and after[1] - before[1] == (1 if case["fdtype"] == "forward" and not case["fin"] else 0)


# ---- the ends of a solve -----------------------------------------------------------------------------------------------------------------
END = JK._case("tridiag_nl", (1025,), "forward", route="quot", diag=True, restart=5, maxit=200)


@pytest.mark.parametrize("maxit,keep", [(7, False), (7, True), (10, True), (1, True)])
def test_the_iterations_run_out_inside_a_cycle_and_at_its_end(monkeypatch, num_cus, maxit, keep):
    f = _f(END)
    s = _solver(END, f, monkeypatch)
    tr = {}
    want, wst = JK.model(END, num_cus, keep=keep, maxit=maxit, trace=tr)
    got = _run(END, s, f, keep=keep, maxit=maxit)
    assert wst["flags"] == 1 and wst["iterations"] == maxit
    _compare(END, got, want, wst, tr)
    assert np.all(np.isnan(got[0])) != keep


@pytest.mark.parametrize("batch", [1, 3])
def test_every_batch_size_gives_the_same_bits(monkeypatch, num_cus, batch):
    for case in (JK.CONVERGENCE[1], JK.CONVERGENCE[5]):          # three cycles of five; seven of two
        f = _f(case)
        s = _solver(case, f, monkeypatch, batch=batch)
        tr = {}
        want, wst = JK.model(case, num_cus, trace=tr)
        assert len(tr["gammas"]) >= 3 and wst["flags"] == 0
        _compare(case, _run(case, s, f), want, wst, tr)


def test_an_rtol_met_by_the_first_column(monkeypatch, num_cus):
    case = JK.CONVERGENCE[0]
    f = _f(case)
    s = _solver(case, f, monkeypatch)
    tr = {}
    want, wst = JK.model(case, num_cus, rtol=0.9, trace=tr)
    assert wst["flags"] == 0 and wst["iterations"] == 1
    _compare(case, _run(case, s, f, rtol=0.9), want, wst, tr)


# ---- failures ------------------------------------------------------------------------------------------------------------------------------
def test_failures_are_arithmetic(monkeypatch, num_cus):
    case = JK._case("lap5_nl", (16, 15), "forward", route="lazy", diag=True, restart=5, maxit=40)
    f = _f(case)
    s = _solver(case, f, monkeypatch)
    _f0, x, b, d = JK.system(case["family"], case["prm"])
    N = x.size
    y, st = _run(case, s, f, b=np.zeros(N))[:2]
    assert st == {"flags": 0, "iterations": 0, "resid": 0.0, "bnorm": 0.0} and np.array_equal(y, np.zeros(N))
    bb = b.copy(); bb[3] = np.nan
    y, st = _run(case, s, f, keep=False, b=bb)[:2]
    assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    for bad in (0.0, np.inf):
        dd = d.copy(); dd[11] = bad
        y, st = _run(case, s, f, keep=False, d=dd)[:2]
        assert st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y)), bad
        y, st = _run(case, s, f, keep=True, d=dd)[:2]
        assert st["flags"] == 2 and np.array_equal(y, np.zeros(N))
    xx = x.copy(); xx[5] = np.nan
    want, wst = JK.model(case, num_cus, keep=False, x=xx)
    y, st = _run(case, s, f, keep=False, x=xx)[:2]
    assert st["flags"] == 2 and st["iterations"] == wst["iterations"] and np.all(np.isnan(y))
    y, st = _run(case, s, f, keep=True, x=xx)[:2]
    assert st["flags"] == 2 and np.array_equal(y, np.zeros(N))
    tr = {}                                       # the same solver is clean again on regular values
    want, wst = JK.model(case, num_cus, trace=tr)
    _compare(case, _run(case, s, f), want, wst, tr)


def test_shape_and_argument_errors():
    f = fd.BuiltinF("tridiag", 64)
    s = fd.JfnkSolver(64)
    good = torch.zeros(64, dtype=torch.float64, device="cuda")
    short = torch.zeros(63, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        s.solve(f, good, short, good.clone())
    with pytest.raises(ValueError):
        s.apply(f, short, good, good.clone())
    with pytest.raises(fd.lib.FdError) as e:
        s.apply(f, good, good, good)              # w must not be z
    assert e.value.code == 1
    with pytest.raises(fd.lib.FdError) as e:
        s.basis()                                 # no solve yet
    assert e.value.code == 3
    with pytest.raises(fd.lib.FdError) as e:
        fd.JfnkSolver(64, restart=65)
    assert e.value.code == 1
    with pytest.raises(fd.lib.FdError) as e:
        s.set_options(1.5, 10)
    assert e.value.code == 1
    with pytest.raises(fd.lib.FdError) as e:
        fd.JfnkSolver(64, "complex")
    assert e.value.code == 3 and "complex-mode" in str(e.value)


# ---- a compiled functor --------------------------------------------------------------------------------------------------------------------
TRIDIAG_SRC = """
struct TriNl {
    long long n;
    template <class P> __device__ typename P::value_type operator()(long long i, const P &X) const
    {
        typedef typename P::value_type V;
        const V xm = i > 0 ? X(i - 1) : V(), xc = X(i), xp = i + 1 < n ? X(i + 1) : V();
        return ((xm - (real_t)2 * xc) + xp) + (xc * xc) * xp;
    }
};
"""


def test_a_compiled_functor_gives_its_built_in_twins_bits(monkeypatch):
    import struct
    case = JK._case("tridiag_nl", (1025,), "forward", diag=True, restart=5, maxit=12)
    jf = fd.JitF(TRIDIAG_SRC, "TriNl", 1025, 1025, params=struct.pack("q", 1025))
    twin = _f(case)
    a = _run(case, _solver(case, twin, monkeypatch), twin)
    b = _run(case, _solver(case, jf, monkeypatch), jf)
    assert a[1] == b[1] and a[1]["iterations"] >= 5 and _same(a[0], b[0]) and a[4] == b[4] and _same(a[2][:a[4]], b[2][:b[4]])
    launcher = (jf.fn, jf.fctx)                   # a raw launcher plus context
    c = _run(case, _solver(case, twin, monkeypatch), launcher)
    assert c[1] == a[1] and _same(c[0], a[0])


# ---- the shared host loop: the sparse consumer's GMRES still equals its model --------------------------------------------------------------
@pytest.mark.parametrize("name,restart", [("1025", 30), ("lap5", 5)])
def test_the_sparse_consumers_gmres_is_unchanged(name, restart):
    import test_gpu_cscgmres as T
    colptr, rowval, N, nz, b, gamma, rl = T.system(name)
    tr = {}
    want, wst = G.solve(rl, 1.0, -gamma, nz, b, 1e-10, 400, restart=restart, trace=tr)
    s = T._solver(colptr, rowval, N)
    s.set_method("gmres", restart)
    got, st = T._device_solve(s, nz, b, 1.0, -gamma, 1e-10, 400)
    V, H, k = s.gmres_basis()
    assert st == wst and wst["flags"] == 0 and _same(got, want)
    assert k == tr["len"] and _same(V.cpu().numpy()[:k], tr["V"][:k]) and _same(H.cpu().numpy()[:k], tr["H"][:k])


# ---- the C client ----------------------------------------------------------------------------------------------------------------------------
def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "jfnk_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "jfnk_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "jfnk: gmres(30): status 0" in out.stdout and "base evaluations 1" in out.stdout and "jfnk: PASS" in out.stdout, out.stdout
