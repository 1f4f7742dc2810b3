"""The finite-difference JVP (csrc/fdjac_jvp.hip: fd_jvp, fd_jvp_async; the lazy JVP kernels of csrc/fdjac_f_jvp.hip) against the
exact host model (tests/jvp_model.py), bit for bit, on every route: the fused small launch, the materialised points paired and scalar,
the lazy launchers' values and finished quotient, a launcher that declines (FD_LAZY_DECLINED -- no built-in launcher can, so a ctypes
callback does), host staging, fd_jvp_async and a second call on the same cache.  The step size is compared with the model's in the
summation order of the route that ran (k_jvp_small / k_dot_partial<false> / k_dot_partial<true> + k_jvp_eps, on the grid the device's
own CU count gives), every value through exact_model.same_bits (a NaN matches any NaN), and every case asserts its route by the
launcher's counts.  The cases live in tests/jvp_cases.py (pure numpy: tests/test_jvp_model_cpu.py evaluates the model on every one of
them on the CPU)."""
import ctypes

import numpy as np
import pytest

import exact_model as X
import jvp_cases as C
import finitediff_jl_amd as fd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -12345.5
FD_LAZY_DECLINED = 100


class _Declining:
    """A BuiltinF behind a lazy JVP launcher that always declines: fn / fctx are the family's own, the launcher a host callback."""

    def __init__(self, f, caps):
        self.f, self.ctx, self.dtype, self.fn, self.fctx = f, f.ctx, f.dtype, f.fn, f.fctx
        self.lazy_jvp_caps = caps
        self.called = []

        def decline(fctx, fx, points, fx_stride, stream):
            self.called.append((bool(points.contents.base_out), bool(points.contents.quotient_out), points.contents.central))
            return FD_LAZY_DECLINED
        self.lazy_jvp_fn = fd.lib.F_LAUNCH_LAZY_JVP(decline)


def _builtin(case, dtype):
    if case["family"] == "sparse":
        return fd.BuiltinF.sparse(*C.pattern(case["prm"][0]), dtype=dtype)
    return fd.BuiltinF(case["family"], *case["prm"], dtype=dtype)


def _device(a, off, t, pad=3):
    """A device copy of `a` inside a sentinel-filled buffer: `off` = 2 keeps it aligned to a pair, 1 breaks that."""
    buf = torch.full((a.size + pad + off,), SENTINEL, dtype=t, device="cuda")
    buf[off:off + a.size] = torch.as_tensor(a, device="cuda")
    return buf, buf[off:off + a.size]


def _guards_intact(buf, off, n):
    h = buf.cpu().numpy()
    return bool((h[:off] == SENTINEL).all() and (h[off + n:] == SENTINEL).all())


@pytest.fixture(scope="module")
def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count      # what fd_ctx holds: the grid of the large dot kernels


@pytest.mark.parametrize("case", C.CASES, ids=[c["id"] for c in C.CASES])
def test_jvp_against_the_exact_model(monkeypatch, num_cus, case):
    if case["small_off"]:
        monkeypatch.setenv("FDJAC_SMALL", "0")            # read when the plan is created: before the cache's first call
    else:
        monkeypatch.delenv("FDJAC_SMALL", raising=False)
    monkeypatch.delenv("FDJAC_LAZY_DIFF", raising=False)
    dtype = C.np_dtype(case)
    t = torch.float64 if dtype == np.float64 else torch.float32
    fdtype, form = case["fdtype"], case["form"]
    route, order = C.route(case), C.dot_order(case)
    builtin = _builtin(case, dtype)
    f = _Declining(builtin, fd.lib.LAZY_JVP_CAP_QUOTIENT if case["quotient"] else 0) if case["declined"] else builtin
    assert (builtin.lazy_jvp_fn is not None) == C.has_lazy(case)
    cache = None
    for call in range(2 if form == "reuse" else 1):
        inp = C.inputs(case, call)
        M, N, x, v, f_in = inp["M"], inp["N"], inp["x"], inp["v"], inp["f_in"]
        want, eps, _dot = C.model(case, num_cus, call)
        if cache is None:
            cache = fd.JVPCache(x if form == "host" else torch.empty(N, dtype=t, device="cuda"), fdtype, lazy=case["lazy"] or case["declined"],
                                quotient=case["quotient"])
        kw = dict(relstep=inp["rel"], absstep=inp["ab"], dir=inp["dir"])
        before = builtin.counts()
        if form == "host":
            xh, vh, fh = x.copy(), v.copy(), None if f_in is None else f_in.copy()
            out = np.full(M, np.nan, dtype)
            fd.finite_difference_jvp_b(out, f, xh, vh, cache, fh, **kw)
            got = out
            assert X.same_bits(xh, x).all() and X.same_bits(vh, v).all() and (f_in is None or X.same_bits(fh, f_in).all())
        else:
            xb, xd = _device(x, 2 - case["xoff"], t)
            vb, vd = _device(v, 2 - case["xoff"], t)
            ob, od = _device(np.full(M, np.nan, dtype), 2 - case["outoff"], t)
            fb, fdv = _device(f_in, 2, t) if f_in is not None else (None, None)
            pair = 2 * np.dtype(dtype).itemsize
            assert (xd.data_ptr() % pair != 0) == bool(case["xoff"]) and (vd.data_ptr() % pair != 0) == bool(case["xoff"])
            assert (od.data_ptr() % pair != 0) == bool(case["outoff"])
            torch.cuda.synchronize()
            fd.finite_difference_jvp_b(od, f, xd, vd, cache, fdv, sync=form != "async", **kw)
            if form == "async":
                builtin.ctx.synchronize()
                e = ctypes.c_double()
                fd.lib.check(fd.lib.typed(builtin.ctx.L, dtype).fd_jvp_get_epsilon(cache._plan[1], ctypes.byref(e)))
                cache.last_epsilon = e.value
            got = od.cpu().numpy()
            # the inputs are unchanged, nothing is written outside out (the element in front of an unaligned out keeps its sentinel)
            assert X.same_bits(xd.cpu().numpy(), x).all() and X.same_bits(vd.cpu().numpy(), v).all()
            assert _guards_intact(xb, 2 - case["xoff"], N) and _guards_intact(vb, 2 - case["xoff"], N)
            assert _guards_intact(ob, 2 - case["outoff"], M), "a store outside out"
            assert fb is None or (X.same_bits(fdv.cpu().numpy(), f_in).all() and _guards_intact(fb, 2, M))
        # the step size, in the summation order of the route that ran
        got_eps = np.array(cache.last_epsilon, dtype=np.float64).astype(dtype)
        assert X.same_bits(got_eps, np.array(eps)).all(), (case["id"], order, float(got_eps), float(eps))
        # the values
        if case["all_nan"]:
            assert np.isnan(want).all()
        else:
            assert np.isfinite(want).mean() >= C.MIN_FINITE and np.isfinite(eps) and eps != 0
        same = X.same_bits(got, want)
        bad = np.nonzero(~same)[0]
        assert same.all(), (case["id"], route, "%d of %d differ, first at %d: got %r, want %r" %
                            (bad.size, M, bad[0], got[bad[0]], want[bad[0]]))
        # which route ran
        after = builtin.counts()
        assert (after[0] - before[0], after[1] - before[1]) == C.counts(case), (case["id"], route, before, after)
        if case["declined"]:
            central = fdtype == "central"
            fin = f_in is not None and not central
            q = bool(case["quotient"]) and not fin and not case["outoff"]
            assert f.called == [(not central and not fin and not q, q, int(central))] * (call + 1), f.called
