"""The matrix-free consumer preconditioned by a LAGGED stored Jacobian on the device (fd_jfnk_solver_set_csc_preconditioner on a
factorisation of fd_csc_solver_factor_async): every solve BIT FOR BIT against the numpy model (tests/jfnk_pc_model.py) on y, flags,
iterations, estimate, ||b||, the last cycle's V and H and its length, over the covering set of tests/jfnk_pc_cases.py -- the
factorisation always from another point and another shift than the solve's; the batch sizes, the ends of a solve, a bad-pivot
factorisation, the setter's errors and the generation rule, the counts, that the preconditioner pays as the model says it does, the
whole sequence from a JacobianCache's nzval, and the plain-C client."""
import os
import subprocess

import numpy as np
import pytest

import finitediff_jl_amd as fd
import jfnk_cases as JK
import jfnk_model as JM
import jfnk_pc_cases as PC
import test_gpu_jfnk as TJ
import test_jfnk_pc_model_cpu as CPU

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CANARY = TJ.CANARY
ROOT = TJ.ROOT
_same, _dev = TJ._same, TJ._dev


@pytest.fixture(scope="module")
def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _select(s, kind):
    if kind[0] == "jacobi":
        s.set_preconditioner("jacobi")
    elif kind[0] == "block":
        s.set_preconditioner("block_jacobi", kind[1])
    else:
        s.set_block_ilu(kind[1])


def _pc(family, prm, kind, nz=None, alpha0=1.0, beta0=-PC.GAMMA0, dtype=np.float64):
    """A sparse consumer on the family's pattern with `kind` selected and the lagged factorisation in it."""
    colptr, rowval, rl, _x0, nz0 = PC.stored(family, prm)
    pc = fd.CscSolver((colptr, rowval, rl.N), dtype=dtype, idx_base=0)
    _select(pc, kind)
    pc.factor(torch.as_tensor(np.ascontiguousarray((nz0 if nz is None else nz).astype(dtype)), device="cuda"), alpha0, beta0)
    return pc


def _run(case, s, f, pc, keep=True, maxit=None, rtol=None, x=None, gamma=PC.GAMMA, b=None):
    """One device solve of the case with pc lent (None: as the solver stands): (y, status, V, H, len, counts before and after)."""
    _f0, x0, b0, _d = JK.system(case["family"], case["prm"])
    x, b = (x0 if x is None else x), (b0 if b is None else b)
    N = x.size
    _xb, xd = _dev(x, 1 - case["xoff"])
    _bb, bd = _dev(b, 1)
    assert (xd.data_ptr() % 16 == 0) == (not case["xoff"])
    ybuf, yd = _dev(np.full(N, CANARY), 1)
    s.set_options(case["rtol"] if rtol is None else rtol, case["maxit"] if maxit is None else maxit)
    s.set_policy(keep)
    if pc is not None:
        s.set_preconditioner(pc)
    fin = TJ._fx(f, xd) if case["fin"] and case["fdtype"] == "forward" else None
    before = s.counts()
    s.solve(f, xd, bd, yd, 1.0, -gamma, f_in=fin)
    st = s.status()
    V, H, k = s.basis()
    assert TJ._canaries_ok(ybuf, 1, N)
    return yd.cpu().numpy(), st, V.cpu().numpy(), H.cpu().numpy(), k, before, s.counts()


def _compare(case, got, want, wst, tr):
    y, st, V, H, k, before, after = got
    print(case["id"], st, wst, "len", k, tr["len"])
    assert st == wst
    assert _same(y, want)
    assert k == tr["len"] and _same(V[:k], tr["V"][:k]) and _same(H[:k], tr["H"][:k])
    base = 1 if (case["fdtype"] == "forward" and not case["fin"]) else 0
    assert after[1] - before[1] == base and after[0] - before[0] >= tr["applications"]


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c["id"])
def test_solve_equals_the_model_bit_for_bit(monkeypatch, num_cus, case):
    f = TJ._f(case)
    s = TJ._solver(case, f, monkeypatch)
    pc = _pc(case["family"], case["prm"], case["kind"])
    assert pc.factor_status() == {"flags": 0}
    tr = {}
    want, wst = PC.model(case, num_cus, trace=tr)
    got = _run(case, s, f, pc)
    _compare(case, got, want, wst, tr)
    again = _run(case, s, f, pc)                  # the one factorisation serves every following solve: the same bits
    assert again[1] == got[1] and _same(again[0], got[0])


THREE_CYCLES = [PC._case("tridiag_nl", (1025,), ("block", 5), "central", route="lazy", restart=2, maxit=200, rtol=1e-9),
                PC._case("lap5_nl", (16, 15), ("ilu", 64), "forward", route="quot", restart=1, maxit=200, rtol=1e-9)]


@pytest.mark.parametrize("batch", [1, 3])
def test_every_batch_size_gives_the_same_bits(monkeypatch, num_cus, batch):
    for case in THREE_CYCLES:
        f = TJ._f(case)
        s = TJ._solver(case, f, monkeypatch, batch=batch)
        tr = {}
        want, wst = PC.model(case, num_cus, trace=tr)
        assert len(tr["gammas"]) >= 3 and wst["flags"] == 0
        _compare(case, _run(case, s, f, _pc(case["family"], case["prm"], case["kind"])), want, wst, tr)


END = PC._case("tridiag_nl", (1025,), ("ilu", 64), "forward", route="quot", restart=5, maxit=200, rtol=0.0)


@pytest.mark.parametrize("maxit,keep", [(7, False), (7, True), (10, True), (1, True)])
def test_the_iterations_run_out_inside_a_cycle_and_at_its_end(monkeypatch, num_cus, maxit, keep):
    f = TJ._f(END)
    s = TJ._solver(END, f, monkeypatch)
    tr = {}
    want, wst = PC.model(END, num_cus, keep=keep, maxit=maxit, trace=tr)
    got = _run(END, s, f, _pc(END["family"], END["prm"], END["kind"]), keep=keep, maxit=maxit)
    assert wst["flags"] == 1 and wst["iterations"] == maxit
    _compare(END, got, want, wst, tr)
    assert np.all(np.isnan(got[0])) != keep


def test_counts_are_steps_plus_restarts_exactly_as_without_a_preconditioner(monkeypatch):
    """rtol = 0: nothing converges, so the host enqueues max_iterations steps and one explicit residual per cycle end, with pc or not."""
    for kind in (("jacobi",), ("block", 32), ("ilu", 64)):
        f = TJ._f(END)
        with_pc, without = TJ._solver(END, f, monkeypatch), TJ._solver(END, f, monkeypatch)
        a = _run(END, with_pc, f, _pc(END["family"], END["prm"], kind), maxit=12)
        b = _run(END, without, f, None, maxit=12)
        assert a[1]["iterations"] == b[1]["iterations"] == 12
        assert a[6][0] - a[5][0] == b[6][0] - b[5][0] == 12 + 3          # cycles of 5, 5 and 2
        assert a[6][1] - a[5][1] == b[6][1] - b[5][1] == 1


@pytest.mark.parametrize("kind", [("jacobi",), ("block", 2), ("ilu", 2)], ids=lambda k: "".join(map(str, k)))
def test_a_bad_pivot_factorisation_ends_every_solve_at_once(monkeypatch, num_cus, kind):
    case = PC._case("tridiag_nl", (65,), kind, "forward", restart=5, maxit=8)
    colptr, rowval, rl, _x0, nz0 = PC.stored(case["family"], case["prm"])
    cols = np.repeat(np.arange(rl.N), np.diff(colptr))
    nz = nz0.copy()
    for r, c in ((0, 0), (0, 1), (1, 0), (1, 1)):              # block 0 of I - GAMMA0 J becomes [[2, 2], [2, 2]]: two equal rows
        q = np.nonzero((rowval == r) & (cols == c))[0][0]
        nz[q] = (2.0 - (1.0 if r == c else 0.0)) / -PC.GAMMA0
    if kind[0] == "jacobi":
        nz[rl.diag[7]] = 1.0 / PC.GAMMA0                       # (the diagonal sees no equal rows: a zero diagonal)
    f = TJ._f(case)
    s = TJ._solver(case, f, monkeypatch)
    pc = _pc(case["family"], case["prm"], kind, nz=nz)
    assert pc.factor_status() == {"flags": 2}
    want, wst = PC.model(case, num_cus, keep=False, lagged=(1.0, -PC.GAMMA0, nz))
    y, st = _run(case, s, f, pc, keep=False)[:2]
    assert st == wst and st["flags"] == 2 and st["iterations"] == 0 and np.all(np.isnan(y))
    y, st = _run(case, s, f, pc, keep=True)[:2]
    assert st["flags"] == 2 and np.array_equal(y, np.zeros(rl.N))
    pc.factor(torch.as_tensor(nz0, device="cuda"), 1.0, -PC.GAMMA0)          # a good factorisation on the same handle: clean again
    tr = {}
    want, wst = PC.model(case, num_cus, trace=tr)
    _compare(case, _run(case, s, f, pc), want, wst, tr)


def test_setter_errors_and_clearing_restores_todays_bits(monkeypatch, num_cus):
    case = PC._case("tridiag_nl", (1025,), ("block", 5), "forward", route="lazy", restart=5, maxit=12)
    plain = dict(JK._case("tridiag_nl", (1025,), "forward", route="lazy", restart=5, maxit=12))
    f = TJ._f(case)
    s = TJ._solver(case, f, monkeypatch)
    with pytest.raises(fd.lib.FdError) as e:                   # wrong N
        s.set_preconditioner(_pc("tridiag_nl", (1023,), ("block", 5)))
    assert e.value.code == 2
    with pytest.raises(fd.lib.FdError) as e:                   # a Float32 handle
        s.set_preconditioner(_pc("tridiag_nl", (1025,), ("block", 5), dtype=np.float32))
    assert e.value.code == 1
    with pytest.raises(TypeError):
        s.set_preconditioner(object())
    pc = _pc(case["family"], case["prm"], case["kind"])
    _db, dd = _dev(JK.system(case["family"], case["prm"])[3], 1)
    s.set_diagonal(dd)
    with pytest.raises(fd.lib.FdError) as e:                   # a diagonal is set
        s.set_preconditioner(pc)
    assert e.value.code == 1
    s.set_diagonal(None)
    s.set_preconditioner(pc)
    with pytest.raises(fd.lib.FdError) as e:                   # ... and the reverse
        s.set_diagonal(dd)
    assert e.value.code == 1
    s.set_diagonal(None)                                       # clearing what is clear is no error
    tr = {}
    want, wst = PC.model(case, num_cus, trace=tr)
    _compare(case, _run(case, s, f, None), want, wst, tr)      # (pc is set)
    s.set_preconditioner(None)
    never = TJ._solver(plain, f, monkeypatch)                  # a solver that never had a preconditioner
    a, b = TJ._run(plain, s, f), TJ._run(plain, never, f)
    tr = {}
    want, wst = JK.model(plain, num_cus, trace=tr)
    assert a[1] == b[1] == wst and _same(a[0], b[0]) and _same(a[0], want)
    assert a[4] == b[4] and _same(a[2][:a[4]], b[2][:b[4]]) and _same(a[3][:a[4]], b[3][:b[4]])
    assert a[6][0] - a[5][0] == b[6][0] - b[5][0]


def test_no_factorisation_and_a_stale_one_are_refused_before_anything_is_enqueued(monkeypatch):
    case = PC._case("tridiag_nl", (257,), ("ilu", 64), "forward", restart=5, maxit=8)
    f = TJ._f(case)
    s = TJ._solver(case, f, monkeypatch)
    colptr, rowval, rl, _x0, nz0 = PC.stored(case["family"], case["prm"])
    pc = fd.CscSolver((colptr, rowval, rl.N), idx_base=0)
    pc.set_block_ilu(64)
    s.set_preconditioner(pc)
    before = s.counts()
    with pytest.raises(fd.lib.FdError) as e:
        _run(case, s, f, None)
    assert e.value.code == 3 and s.counts() == before          # no factorisation: nothing enqueued, not even f(x)
    nzd = torch.as_tensor(nz0, device="cuda")
    pc.factor(nzd, 1.0, -PC.GAMMA0)
    good = _run(case, s, f, None)
    assert good[1]["flags"] == 0
    bd = torch.as_tensor(JK.system(case["family"], case["prm"])[2], device="cuda")
    pc.solve(nzd, bd, torch.empty_like(bd), 1.0, -PC.GAMMA0)   # the lent handle solves: its buffers are that solve's now
    before = s.counts()
    with pytest.raises(fd.lib.FdError) as e:
        _run(case, s, f, None)
    assert e.value.code == 9 and "stale" in str(e.value) and s.counts() == before
    pc.factor(nzd, 1.0, -PC.GAMMA0)
    again = _run(case, s, f, None)
    assert again[1] == good[1] and _same(again[0], good[0])


def test_the_lagged_factorisation_pays_as_the_model_says(monkeypatch, num_cus):
    """The device's counts are the model's; the true residual against jacobian_dense at x1 is within 10 x rtol.  (The margin of
    profiles/jfnk_accuracy.md is 4 x the model's own true residual; the device equals the model bit for bit, so it holds a fortiori and
    is asserted too.)"""
    H = CPU.HELP
    f, _x0, x1, b, rl, colptr, rowval, nz0 = CPU.help_system()
    (y0, s0), (y1, s1, tr) = CPU.help_models(num_cus)
    case = PC._case(H["family"], H["prm"], H["kind"], H["fdtype"], restart=H["restart"], maxit=H["maxit"], rtol=H["rtol"])
    fdev = TJ._f(case)
    pc = fd.CscSolver((colptr, rowval, rl.N), idx_base=0)
    pc.set_block_ilu(H["kind"][1])
    pc.factor(torch.as_tensor(nz0, device="cuda"), 1.0, -H["gamma"])
    without = _run(case, TJ._solver(case, fdev, monkeypatch), fdev, None, x=x1, gamma=H["gamma"], b=b)
    with_pc = _run(case, TJ._solver(case, fdev, monkeypatch), fdev, pc, x=x1, gamma=H["gamma"], b=b)
    print("steps without", without[1]["iterations"], "with", with_pc[1]["iterations"])
    assert without[1] == s0 and with_pc[1] == s1 and _same(without[0], y0) and _same(with_pc[0], y1)
    assert (s0["iterations"], s1["iterations"]) == (H["steps_without"], H["steps_with"]) and s0["flags"] == s1["flags"] == 0
    res = JM.true_residual(H["family"], H["prm"], x1, 1.0, -H["gamma"], b, with_pc[0])
    model_res = JM.true_residual(H["family"], H["prm"], x1, 1.0, -H["gamma"], b, y1)
    print("true residual %.3e (model %.3e)" % (res, model_res))
    assert res <= 10 * H["rtol"] and res <= 4 * model_res


def test_end_to_end_from_a_jacobian_caches_nzval():
    nx, ny = 16, 15
    N = nx * ny
    P = fd.patterns
    colptr, rowval = P.lap5_csc(nx, ny)
    _f0, x0, b, _d = JK.system("lap5_nl", (nx, ny))
    x1 = x0 + PC.LAG * np.random.default_rng(9).random(N)
    f = fd.BuiltinF("lap5_nl", nx, ny)
    x0d, x1d, bd = (torch.as_tensor(a, device="cuda") for a in (x0, x1, b))
    J = fd.SparseMatrixCSC(N, N, colptr, rowval, torch.zeros(rowval.size, dtype=torch.float64, device="cuda"))
    cache = fd.JacobianCache(x0d.clone(), "forward", colorvec=P.lap5_colors(nx, ny), sparsity=J)
    fd.finite_difference_jacobian_b(J, f, x0d, cache)          # 1. J(x0), stored
    pc = fd.CscSolver(J)
    pc.set_block_ilu(256)                                      # 2.
    pc.factor(J, 1.0, -PC.GAMMA)
    assert pc.factor_status() == {"flags": 0}
    s = fd.JfnkSolver(N, "forward", 30)
    s.set_options(1e-8, 200)
    plain = fd.JfnkSolver(N, "forward", 30)
    plain.set_options(1e-8, 200)
    s.set_preconditioner(pc)                                   # 3.
    for xd, x in ((x0d, x0), (x1d, x1)):                       # 4.
        y, y2 = torch.empty_like(bd), torch.empty_like(bd)
        s.solve(f, xd, bd, y, 1.0, -PC.GAMMA)
        plain.solve(f, xd, bd, y2, 1.0, -PC.GAMMA)
        st, st2 = s.status(), plain.status()
        print(st, st2)
        assert st["flags"] == 0 and st2["flags"] == 0 and 1 <= st["iterations"] < st2["iterations"]
        assert JM.true_residual("lap5_nl", (nx, ny), x, 1.0, -PC.GAMMA, b, y.cpu().numpy()) <= 1e-6


def test_plain_c_client_builds_and_runs(tmp_path):
    exe = str(tmp_path / "jfnk_precond_client")
    libdir = os.path.join(ROOT, "finitediff.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "jfnk_precond_client.c"), "-o", exe, "-L" + libdir, "-lfdjac", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "jfnk_precond: factor status 0" in out.stdout and "lagged block ILU : x0 status 0" in out.stdout and "jfnk_precond: PASS" in out.stdout, out.stdout
