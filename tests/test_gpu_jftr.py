"""The matrix-free trust-region consumer on the device (csrc/fdjac_jftr.hip, fd_jftr_*): every step BIT FOR BIT against the numpy model
(tests/jftr_model.py) on y, r_out, exit, flags, iterations, the four status scalars and the counts, over the covering set of
tests/jftr_cases.py; the operator alone against torch's lam v + beta q with q from the public fd_jvp_async; the exits, the failures, the
batch sizes, the large kernels at small sizes and the unfused pair (a child process), the stored trust-region consumer beside it, the
path end to end beside a JacobianCache's stored J, and the plain-C client."""
import os
import subprocess
import sys

import numpy as np
import pytest

import finitediff_jl_amd as fd
import csc_tr_model as TM
import jftr_cases as K
import test_csctr_model_cpu as H
import test_jftr_model_cpu as CPU

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CANARY = 7.25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _the_library_has_the_consumer():
    """Every test here describes fd_jftr_*: where the consumer is missing, each of them fails."""
    assert hasattr(fd.lib.load(), "fd_jftr_step_async") and hasattr(fd, "JfTrustRegion")


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


def _consumer(case, f, monkeypatch, batch=None):
    assert not case["small_off"] and case["fuse"]          # (those run in tests/jftr_switch_child.py)
    monkeypatch.setenv("FDJAC_SMALL", "1")
    monkeypatch.setenv("FDJAC_JFTR_FUSE", "1")
    if batch is not None:
        monkeypatch.setenv("FDJAC_CSC_BATCH", str(batch))
    s = fd.JfTrustRegion(K.size_of(case["family"], case["prm"]), case["fdtype"])
    s.set_lazy(f if case["route"] != "plain" else None, quotient=case["route"] == "quot")
    return s


def _fx(f, xd):
    """f(x) on the device by one plain launch of the family's own launcher."""
    out = torch.empty_like(xd)
    n = xd.numel()
    rc = f.fn(f.fctx, out.data_ptr(), xd.data_ptr(), 1, n, n, 0, n, 0, f.ctx.stream)
    assert rc == 0
    return out


def _run(case, s, f, num_cus, keep=True, maxit=None, x=None, g=None, m=None, radius=None, with_r=True):
    """One device step of the case: (y, r_out, status, applications used, base evaluations)."""
    _f0, x0, g0, m0 = K.operands(case)
    x, g, m = (x0 if x is None else x), (g0 if g is None else g), (m0 if m is None else m)
    N = x.size
    xoff, moff = 1 - case["xoff"], 1 - case["moff"]          # (the canary takes one element: an odd offset is the aligned one)
    xbuf, xd = _dev(x, xoff)
    _gb, gd = _dev(g, 1)
    mbuf, md = _dev(m, moff)
    assert (xd.data_ptr() % 16 == 0) == (not case["xoff"]) and (md.data_ptr() % 16 == 0) == (not case["moff"])
    ybuf, yd = _dev(np.full(N, CANARY), 1)
    rbuf, rd = _dev(np.full(N, CANARY), 0)
    s.set_options(case["rtol"], case["maxit"] if maxit is None else maxit)
    s.set_policy(keep)
    s.set_diagonal(md if case["diag"] else None)
    fin = _fx(f, xd) if case["fin"] and case["fdtype"] == "forward" else None
    before = s.counts()
    s.step(f, xd, gd, yd, K.radius_of(case, num_cus) if radius is None else radius, case["lam"], case["beta"], f_in=fin, r_out=rd if with_r else None)
    st = s.status()
    after = s.counts()
    assert _canaries_ok(ybuf, 1, N) and _canaries_ok(rbuf, 0, N)
    assert _canaries_ok(xbuf, xoff, N) and _same(xd.cpu().numpy(), x) and _same(md.cpu().numpy(), m) and _same(gd.cpu().numpy(), g)      # x and its surroundings
    return yd.cpu().numpy(), rd.cpu().numpy(), st, after[0] - before[0], after[1] - before[1]


def _compare(case, got, want, cnt):
    y, r, st, apps, base = got
    wy, wr, wst = want
    print(case["id"], st, wst, "applications", apps, cnt["applications"])
    assert TM.same_status(st, wst)
    assert _same(y, wy) and _same(r, wr)
    assert apps == cnt["applications"] and base == (1 if (case["fdtype"] == "forward" and not case["fin"]) else 0)


def _model(case, num_cus, **kw):
    cnt = {}
    return K.model(case, num_cus, counts=cnt, **kw), cnt


def test_the_cases_cover():
    sizes = {K.size_of(c["family"], c["prm"]) for c in K.CASES}
    for n in K.TILE_SIZES + K.SWITCH_SIZES:
        assert n in sizes, n
    for grid in K.LAP5_GRIDS:
        for fam in ("lap5", "lap5_nl"):
            assert any(c["family"] == fam and c["prm"] == grid for c in K.CASES), (fam, grid)
    assert {K.size_of(c["family"], c["prm"]) for c in K.SWITCHED if c["small_off"] and c["fuse"]} == {1, 2, 3, 257, 1025}
    both = {False, True}
    for fam in K.FAMILIES:          # every route on EACH family
        mine = [c for c in K.CASES if c["family"] == fam]
        assert {c["fdtype"] for c in mine} == {"forward", "central"}, fam
        assert {bool(c["fin"]) for c in mine if c["fdtype"] == "forward"} == both, fam          # (the central arm never reads f_in)
        assert {c["route"] for c in mine} == {"plain", "lazy", "quot"}, fam
        for key in ("diag", "xoff"):
            assert {bool(c[key]) for c in mine} == both, (fam, key)
        assert {bool(c["moff"]) for c in mine if c["diag"]} == both, fam
    big = [c for c in K.CASES if K.size_of(c["family"], c["prm"]) > 16384]
    assert {(c["fdtype"], c["route"]) for c in big} == {(a, r) for a in ("forward", "central") for r in ("plain", "lazy", "quot")}
    odd = [c for c in big if K.size_of(c["family"], c["prm"]) % 2 == 1]
    assert any(c["xoff"] for c in odd) and any(not c["xoff"] for c in odd)                      # k_jt_p<false> and <true> with the odd tail
    assert any(c["xoff"] for c in big if c not in odd)
    assert any(c["diag"] and c["moff"] for c in big) and any(not c["diag"] for c in big)
    # every exit, both norms, small and above kSmallN; a boundary exit behind several fused direction updates
    for c in K.EXITS:
        assert K.model(c)[2]["exit"] == K.WANT_EXIT[(c["lam"], c["beta"], c["radius"])], c["id"]
    for small in both:
        mine = [c for c in K.EXITS if (K.size_of(c["family"], c["prm"]) <= 16384) == small]
        assert {(K.WANT_EXIT[(c["lam"], c["beta"], c["radius"])], c["diag"]) for c in mine} == {(e, d) for e in range(4) for d in both}
    assert any(K.model(c)[2]["exit"] == 1 and K.model(c)[2]["iterations"] >= 3 for c in big)
    assert any(K.model(c)[2]["exit"] == 0 and K.model(c)[2]["flags"] == 0 and K.model(c)[2]["iterations"] >= 20 for c in K.EXITS[14:])
    assert 70 <= len(K.CASES) <= 90


@pytest.mark.parametrize("case", K.CASES + K.EXITS, ids=lambda c: c["id"])
def test_step_equals_the_model_bit_for_bit(monkeypatch, num_cus, case):
    f = _f(case)
    s = _consumer(case, f, monkeypatch)
    want, cnt = _model(case, num_cus)
    got = _run(case, s, f, num_cus)
    _compare(case, got, want, cnt)
    again = _run(case, s, f, num_cus, with_r=False)          # a second step on the handle, without r_out: the same bits
    assert TM.same_status(again[2], got[2]) and _same(again[0], got[0]) and again[3] == got[3]
    if case in K.EXITS:
        wst = want[2]
        assert wst["exit"] == K.WANT_EXIT[(case["lam"], case["beta"], case["radius"])] and wst["flags"] == (2 if wst["exit"] == 3 else 0)
        if wst["exit"] in (1, 2):
            delta = K.radius_of(case, num_cus)
            assert abs(got[2]["step_norm"] - delta) <= 1e-12 * delta


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c["id"])
def test_apply_equals_torch_on_the_public_jvp(monkeypatch, case):
    """w = lam v + beta q with q from fd_jvp_async(f_in = f(x)): no numpy model in this oracle."""
    f = _f(case)
    s = _consumer(case, f, monkeypatch)
    _f0, x, _g, _m = K.operands(case)
    N = x.size
    v = np.random.default_rng(N + 5).uniform(-1.0, 1.0, N)
    _xb, xd = _dev(x, 1 - case["xoff"])
    _vb, vd = _dev(v, 1 - case["moff"])
    wbuf, wd = _dev(np.full(N, CANARY), 1 - (case["xoff"] ^ case["moff"]))
    fx = _fx(f, xd)
    lam, beta = 0.75, -0.3
    before = s.counts()
    s.apply(f, xd, vd, wd, lam, beta, f_in=fx if case["fin"] else None)
    after = s.counts()
    q = torch.empty(N, dtype=torch.float64, device="cuda")
    cache = fd.JVPCache(xd, case["fdtype"], lazy=case["route"] != "plain", quotient=False)
    fd.finite_difference_jvp_b(q, f, xd, vd, cache, f_in=fx, sync=False)
    want = lam * vd + beta * q
    torch.cuda.synchronize()
    assert _same(wd.cpu().numpy(), want.cpu().numpy())
    assert _canaries_ok(wbuf, 1 - (case["xoff"] ^ case["moff"]), N)
    assert after[0] - before[0] == 1 and after[1] - before[1] == (1 if case["fdtype"] == "forward" and not case["fin"] else 0)


# ---- the ends of a step ------------------------------------------------------------------------------------------------------------------
END = K._case("lap5", (130, 131), "forward", route="quot", diag=True, model=K.INTERIOR[0])
END_SMALL = K._case("tridiag", (1025,), "central", route="lazy", model=K.INTERIOR[0])


@pytest.mark.parametrize("case", [END, END_SMALL], ids=lambda c: c["id"])
@pytest.mark.parametrize("maxit,keep", [(7, False), (7, True), (8, True), (1, True)])
def test_the_iterations_run_out_with_both_policies(monkeypatch, num_cus, case, maxit, keep):
    f = _f(case)
    s = _consumer(case, f, monkeypatch)
    want, cnt = _model(case, num_cus, keep=keep, maxit=maxit)
    assert want[2]["flags"] == 1 and want[2]["iterations"] == maxit
    got = _run(case, s, f, num_cus, keep=keep, maxit=maxit)
    _compare(case, got, want, cnt)
    assert np.all(np.isnan(got[0])) != keep and np.all(np.isnan(got[1])) != keep


@pytest.mark.parametrize("batch", [1, 8])
def test_every_batch_size_gives_the_same_bits(monkeypatch, num_cus, batch):
    """Interior runs of 21 and 28 iterations and a boundary exit after 3 end in the middle of a batch of 8: the kernels enqueued behind
    the end leave on `done` (f! still runs, on scratch)."""
    picks = [K.EXITS[0], K.EXITS[14], [c for c in K.CASES if c["id"].startswith("tridiag_nl-16386-central-plain-l0.5-b-1-r0.5y")][0]]
    for case in picks:
        f = _f(case)
        s = _consumer(case, f, monkeypatch, batch=batch)
        want, cnt = _model(case, num_cus)
        assert want[2]["iterations"] % 8 != 0 and want[2]["flags"] == 0
        _compare(case, _run(case, s, f, num_cus), want, cnt)


def test_the_switched_routes_in_a_child_process():
    """The large kernels at N = 1, 2, 3, 257, 1025 (FDJAC_SMALL=0) and k_tr_p plus the JVP's own dot above kSmallN (FDJAC_JFTR_FUSE=0):
    tests/jftr_switch_child.py, with FDJAC_TEST_SWITCHES=1."""
    env = dict(os.environ, FDJAC_TEST_SWITCHES="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "jftr_switch_child.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout and out.stdout.count(": ok ") == len(K.SWITCHED) and "MISMATCH" not in out.stdout


# ---- failures ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [K._case("lap5_nl", (16, 15), "forward", route="lazy", diag=True, model=K.INTERIOR[0], maxit=40),
                                  K._case("tridiag", (16385,), "central", route="quot", diag=True, moff=1, model=K.INTERIOR[0], maxit=12)],
                         ids=lambda c: c["id"])
def test_failures_are_arithmetic(monkeypatch, num_cus, case):
    f = _f(case)
    s = _consumer(case, f, monkeypatch)
    _f0, x, g, m = K.operands(case)
    N = x.size
    y, r, st, apps, base = _run(case, s, f, num_cus, g=np.zeros(N))
    assert st == {"flags": 0, "exit": 0, "iterations": 0, "resid": 0.0, "g_norm": 0.0, "step_norm": 0.0, "pred": 0.0}
    assert np.array_equal(y, np.zeros(N)) and np.array_equal(r, np.zeros(N)) and apps == 0
    for bad in (0.0, -1.0, np.nan, np.inf):
        mm = m.copy(); mm[11] = bad
        y, r, st, apps, base = _run(case, s, f, num_cus, keep=False, m=mm)
        assert st["flags"] == 2 and st["iterations"] == 0 and st["exit"] == 0 and np.all(np.isnan(y)) and np.all(np.isnan(r)) and apps == 0, bad
        y, r, st, apps, base = _run(case, s, f, num_cus, keep=True, m=mm)
        assert st["flags"] == 2 and np.array_equal(y, np.zeros(N)) and _same(r, g)
    xx = x.copy(); xx[5] = np.nan
    want, cnt = _model(case, num_cus, keep=False, x=xx)
    got = _run(case, s, f, num_cus, keep=False, x=xx)
    assert want[2]["flags"] == 2 and want[2]["iterations"] == 0 and cnt["applications"] == 1
    assert got[2]["flags"] == 2 and got[2]["iterations"] == 0 and np.all(np.isnan(got[0])) and got[3] == 1
    y, r, st, apps, base = _run(case, s, f, num_cus, keep=True, x=xx)
    assert st["flags"] == 2 and np.array_equal(y, np.zeros(N))
    want, cnt = _model(case, num_cus)              # the same consumer is clean again on regular values
    _compare(case, _run(case, s, f, num_cus), want, cnt)


def test_g_may_be_f_in_and_y_or_r_out_may_be_g(monkeypatch, num_cus):
    case = K._case("tridiag", (2049,), "forward", fin=True, route="lazy", diag=True, model=K.BOUNDARY[0])
    f = _f(case)
    s = _consumer(case, f, monkeypatch)
    _f0, x, _g, m = K.operands(case)
    xd, md = torch.as_tensor(x, device="cuda"), torch.as_tensor(m, device="cuda")
    with np.errstate(all="ignore"):
        g = _f0(x)                                 # g = f(x) = f_in
    want, cnt = _model(case, num_cus, g=g)
    delta = K.radius_of(case, num_cus)
    s.set_options(case["rtol"], case["maxit"]); s.set_policy(True); s.set_diagonal(md)
    for alias in ("y", "r"):
        fx = _fx(f, xd)
        assert _same(fx.cpu().numpy(), g)
        other = torch.full_like(fx, CANARY)
        y, r = (fx, other) if alias == "y" else (other, fx)
        s.step(f, xd, fx, y, delta, case["lam"], case["beta"], f_in=fx, r_out=r)
        st = s.status()
        assert TM.same_status(st, want[2]) and _same(y.cpu().numpy(), want[0]) and _same(r.cpu().numpy(), want[1]), alias


def test_shape_and_argument_errors():
    f = fd.BuiltinF("tridiag", 64)
    s = fd.JfTrustRegion(64)
    good = torch.zeros(64, dtype=torch.float64, device="cuda")
    short = torch.zeros(63, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        s.step(f, good, short, good.clone(), 1.0)
    with pytest.raises(ValueError):
        s.apply(f, short, good, good.clone())
    for call in (lambda: s.apply(f, good, good.clone(), good),                     # w must not be x
                 lambda: s.step(f, good, good.clone(), good, 1.0),                 # y must not be x
                 lambda: s.step(f, good, good.clone(), good.clone(), 0.0),         # radius
                 lambda: s.step(f, good, good.clone(), good.clone(), 1.0, lam=-1.0),
                 lambda: s.step(f, good, good.clone(), good.clone(), 1.0, beta=0.0),
                 lambda: s.set_options(1.5, 10)):
        with pytest.raises(fd.lib.FdError) as e:
            call()
        assert e.value.code == 1
    with pytest.raises(fd.lib.FdError) as e:
        fd.JfTrustRegion(64, "complex")
    assert e.value.code == 3 and "complex-mode" in str(e.value)
    assert s.status()["flags"] == 0 and s.counts() == (0, 0)


# ---- beside the stored consumers -------------------------------------------------------------------------------------------------------------
def test_the_stored_trust_region_consumer_is_unchanged_around_a_matrix_free_step(monkeypatch, num_cus):
    name, lam, kind, radius = "spd", 0.0, 1, ("rel", 0.5)
    colptr, rowval, nz, N, g, rl = H.case(name)
    want_y, want_r, wst, _trace = H.model_step(name, lam, kind, radius)
    delta = H.radius_of(name, lam, kind, radius)
    stored = fd.CscTrustRegion((colptr, rowval, N), idx_base=0)
    stored.set_options(H.RTOL, H.MAXIT)
    nzd, gd = torch.as_tensor(nz, device="cuda"), torch.as_tensor(g, device="cuda")

    def stored_step():
        y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        r = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        stored.step(nzd, gd, y, delta, lam, "diag", r_out=r)
        return y.cpu().numpy(), r.cpu().numpy(), stored.status()

    alone = stored_step()
    case = END
    f = _f(case)
    s = _consumer(case, f, monkeypatch)
    want, cnt = _model(case, num_cus)
    _compare(case, _run(case, s, f, num_cus), want, cnt)
    after = stored_step()
    for got in (alone, after):
        assert TM.same_status(got[2], wst) and _same(got[0], want_y) and _same(got[1], want_r)
    assert TM.same_status(alone[2], after[2]) and _same(alone[0], after[0]) and _same(alone[1], after[1])


@pytest.mark.parametrize("fam,prm", [("lap5", (16, 15)), ("tridiag", (1025,))])
def test_end_to_end_beside_a_jacobian_caches_stored_j(fam, prm):
    """The same f!: its J stored through a JacobianCache and handed (negated: B = lam I - J) to CscTrustRegion, and handed as it is to
    JfTrustRegion -- the steps agree to the allowance tests/test_jftr_model_cpu.py measures on the CPU."""
    P = fd.patterns
    N = K.size_of(fam, prm)
    colptr, rowval = P.lap5_csc(*prm) if fam == "lap5" else P.tridiag_csc(N)
    colors = P.lap5_colors(*prm) if fam == "lap5" else P.cyclic_colors(N, 3)
    _f0, x, g, _m = K.system(fam, prm)
    f = fd.BuiltinF(fam, *prm)
    xd, gd = torch.as_tensor(x, device="cuda"), torch.as_tensor(g, device="cuda")
    J = fd.SparseMatrixCSC(N, N, colptr, rowval, torch.zeros(rowval.size, dtype=torch.float64, device="cuda"))
    cache = fd.JacobianCache(xd.clone(), "forward", colorvec=colors, sparsity=J)
    fd.finite_difference_jacobian_b(J, f, xd, cache)
    lam = 0.5
    stored = fd.CscTrustRegion(J)
    free = fd.JfTrustRegion(N, "forward")
    free.set_lazy(f)
    for s in (stored, free):
        s.set_options(CPU.RTOL, K.MAXIT)
    negJ = -J.nzval
    star = None
    for fac in (None, 0.4, 0.1):
        radius = INF if fac is None else fac * star
        ys, yf = torch.empty_like(xd), torch.empty_like(xd)
        stored.step(negJ, gd, ys, radius, lam, "I")
        free.step(f, xd, gd, yf, radius, lam, -1.0)
        ss, sf = stored.status(), free.status()
        if fac is None:
            star = ss["step_norm"]
        err = float(torch.linalg.norm(yf - ys) / torch.linalg.norm(ys))
        print(fam, prm, "radius", radius, ss, sf, "||y_free - y_stored|| / ||y_stored|| = %.3e (allowed %.3e)" % (err, CPU.ALLOWED))
        assert ss["flags"] == sf["flags"] == 0 and ss["exit"] == sf["exit"] == (0 if fac is None else 1) and ss["iterations"] == sf["iterations"]
        assert err <= CPU.ALLOWED


# ---- the C client ----------------------------------------------------------------------------------------------------------------------------
def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "jftr_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "jftr_client.c"),
                           "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no boundary: status 0 exit 0" in out.stdout and "base evaluations 1" in out.stdout and "jftr: PASS" in out.stdout, out.stdout
