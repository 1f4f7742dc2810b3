"""The line-aligned emit of the tridiagonal storing launch (fd_band_emit_wave_lines, include/fdjac_device.h): the launcher places the
first wavefront so that every interior wavefront owns one 128-byte aligned 3072-byte span of a CSC nzval, lane 63 forms the first value
of the next wavefront's first column, and the first / last wavefront of a launch write their columns one by one.  Every stored value
must have the bits of the earlier emit (FDJAC_STORE_LINES=0) and of the hand-over path (FDJAC_LAZY_STORE=0), wherever `out` lies in
memory (the placement depends on its address: for half of the 8-byte offsets no even first column exists and the launch keeps the
earlier emit), for every column window, in the two-launch call and in the fused step; nothing outside `out` may be touched."""
import numpy as np
import pytest

import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [130, 256, 257, 385, 1000, 4099]
PAD = 32                      # canary elements on either side of an output
CANARY = -7.25e300


def _x(N):
    return torch.as_tensor((np.random.default_rng(N).random(N) * 2 - 0.5), device="cuda")


def _placed(n, offset):
    """an output of n elements `offset` elements past a 128-byte line, canaries around it"""
    buf = torch.full((PAD + 16 + n + PAD,), CANARY, dtype=torch.float64, device="cuda")
    lead = (-(buf.data_ptr() // 8)) % 16 + offset
    assert lead < PAD + 16
    out = buf[lead:lead + n]
    assert (out.data_ptr() // 8) % 16 == offset % 16
    out.fill_(float("nan"))
    return buf, out, lead


def _canaries_intact(buf, lead, n):
    return bool((buf[:lead] == CANARY).all()) and bool((buf[lead + n:] == CANARY).all())


def _run(monkeypatch, N, fdtype, family, path, win=None, offset=0, fused=None, calls=1):
    """one Jacobian (or its column window) through `path`: "lines" (the default), "old" (FDJAC_STORE_LINES=0), "handover"
    (FDJAC_LAZY_STORE=0); returns the stored values.  Asserts on the way that x and everything around `out` stay untouched.
    fused = None: the two-launch call with the library's choice of step-size reduction (one workgroup up to N = 16384);
    True / False: the wide reduction at every N (FDJAC_SMALL=0) inside the storing launch / as a launch of its own."""
    monkeypatch.setenv("FDJAC_SMALL", "1" if fused is None else "0")
    monkeypatch.setenv("FDJAC_LAZY_STORE", "0" if path == "handover" else "1")
    monkeypatch.setenv("FDJAC_STORE_LINES", "0" if path == "old" else "1")
    colptr, rowval = P.tridiag_csc(N)
    colors = P.cyclic_colors(N, 3)
    J = fd.SparseMatrixCSC(N, N, colptr, rowval)
    plan = fd.make_plan(J, J, colors, fdtype, col_window=win)
    f = fd.BuiltinF(family, N)
    plan.set_lazy(f, fused=bool(fused))
    # (the plan may withhold the storing launch from a window of a column or two: those go the hand-over way on every path)
    assert plan.info(fd.lib.INFO_LAZY_STORE) == (0 if path == "handover" else 1) or (win is not None and win[1] - win[0] < 128)
    x = _x(N)
    x0 = x.clone()
    n = plan.out_len(0)
    buf, out, lead = _placed(n, offset)
    for _ in range(calls):
        out.fill_(float("nan"))
        plan.enable_timing(2)
        plan.jacobian(f, x, [out])
        tm = plan.timings()
        plan.enable_timing(0)
        if fused is not None:
            assert tm["eps"]["launches"] == (0 if fused else 1), (fused, tm)      # the fused step ran / did not run
    assert torch.equal(x.view(torch.int64), x0.view(torch.int64))
    assert _canaries_intact(buf, lead, n), (N, fdtype, family, path, win, offset)
    assert not torch.isnan(out).any(), (N, fdtype, family, path, win, offset, int(torch.isnan(out).sum()))
    return out.clone().view(torch.int64)


_REF = {}


def _reference(monkeypatch, N, fdtype, family):
    """the hand-over path's bits of the whole Jacobian, computed once per (N, fdtype, family)"""
    key = (N, fdtype, family)
    if key not in _REF:
        _REF[key] = _run(monkeypatch, N, fdtype, family, "handover")
    return _REF[key]


def _same(a, b, what):
    bad = torch.nonzero(a != b).flatten()
    assert a.numel() == b.numel() and bad.numel() == 0, (what, int(bad.numel()), bad[:8].tolist())


@pytest.mark.parametrize("family", ["tridiag", "tridiag_nl"])
@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("N", SIZES)
def test_line_aligned_emit_has_the_bits_of_the_earlier_emit_and_of_the_handover(monkeypatch, N, fdtype, family):
    ref = _reference(monkeypatch, N, fdtype, family)
    assert ref.numel() == 3 * N - 2
    new = _run(monkeypatch, N, fdtype, family, "lines")
    old = _run(monkeypatch, N, fdtype, family, "old")
    _same(new, old, "lines vs old")
    _same(new, ref, "lines vs hand-over")


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("N", [385, 1000])
def test_every_placement_of_out_gives_the_same_bits_and_touches_nothing_else(monkeypatch, N, fdtype):
    # out / 8 mod 16 = 0 .. 15 (and 16 = 0 again): even offsets have an even first column (at or below column 0: the first wavefront
    # starts before the matrix), odd offsets have none and keep the earlier emit
    ref = _reference(monkeypatch, N, fdtype, "tridiag_nl")
    for offset in range(17):
        for path in ("lines", "old"):
            _same(_run(monkeypatch, N, fdtype, "tridiag_nl", path, offset=offset), ref, (path, offset))


WINDOW_SPLITS = [
    [0, 128, 1280, 4099],                 # ends on multiples of the wavefront's 128 columns
    [0, 129, 1283, 2049, 4099],           # ends strictly inside wavefronts, odd and even
    [0, 1, 2, 130, 387, 3971, 4098, 4099],  # windows of one column, of one wavefront and a bit, a last window of one column
    [0, 2048, 2050, 2306, 4099],          # a window shorter than a wavefront, one of exactly two
]


@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("split", range(len(WINDOW_SPLITS)))
def test_column_windows_concatenate_to_the_unsharded_bits(monkeypatch, fdtype, split):
    N = 4099
    ref = _reference(monkeypatch, N, fdtype, "tridiag_nl")
    cuts = WINDOW_SPLITS[split]
    # (entry_begin = 3 a - 1 of a window from column a > 0: whether an even first column exists depends on the parity of
    #  entry_begin - out / 8 -- both parities for every window)
    # None: out 8 bytes before a line -- for an even a > 0 the line-aligned first column is then a ITSELF: the launch's first
    # wavefront starts exactly at the window and no wavefront before it exists to write the window's first value
    for path, parity in (("lines", 0), ("lines", 1), ("lines", None), ("old", 0)):
        parts = [_run(monkeypatch, N, fdtype, "tridiag_nl", path, win=(a, b), offset=15 if parity is None else (6 * k + parity) % 16)
                 for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
        _same(torch.cat(parts), ref, (path, parity, cuts))


@pytest.mark.parametrize("family", ["tridiag", "tridiag_nl"])
@pytest.mark.parametrize("fdtype", ["forward", "central"])
@pytest.mark.parametrize("N", [4099, 2 ** 17])
def test_fused_step_with_line_aligned_emit_has_the_bits_of_the_two_launch_call(monkeypatch, N, fdtype, family):
    two = _run(monkeypatch, N, fdtype, family, "lines", fused=False)
    _same(_run(monkeypatch, N, fdtype, family, "lines", fused=True, calls=2), two, "fused lines")
    _same(_run(monkeypatch, N, fdtype, family, "old", fused=True, calls=2), two, "fused old")
    _same(_run(monkeypatch, N, fdtype, family, "lines", fused=True, offset=6), two, "fused lines, out 48 B past a line")
    _same(_run(monkeypatch, N, fdtype, family, "lines", fused=True, win=(1283, N), offset=3),
          two[3 * 1283 - 1:], "fused lines, window")
