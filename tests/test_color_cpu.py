"""The device column colouring without a GPU: the host model of its contract (tests/color_model.py), the priority function pinned,
and the C ABI / binding / shim of fd_color_columns_device and fd_color_check_device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P

import color_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _patterns():
    yield "tridiagonal 101", 101, 101, *P.tridiag_csc(101)
    yield "5-point 23 x 17", 23 * 17, 23 * 17, *P.lap5_csc(23, 17)
    yield "random 40 x 60", 40, 60, *P.csc_from_dense(cm.random_40x60().astype(float))
    A = np.zeros((3, 7))
    A[1, :] = 1
    yield "dense row 3 x 7", 3, 7, *P.csc_from_dense(A)
    for seed in (1, 2, 3):
        yield "random band seed %d" % seed, 3000, 3000, *cm.random_band(3000, 3000, 6, 300, seed)


@pytest.mark.parametrize("case", list(_patterns()), ids=lambda c: c[0])
def test_model_colouring_is_valid_and_within_the_greedy_bound(case):
    name, M, N, colptr, rowval = case
    colors = cm.greedy(M, N, colptr, rowval)
    delta = cm.max_conflicts(M, N, colptr, rowval)
    assert colors.min() >= 1 and cm.valid(M, colptr, rowval, colors)
    # greedy in ANY order: a column sees at most Delta forbidden colours, so its colour is at most Delta + 1
    assert colors.max() <= delta + 1, (name, int(colors.max()), delta)
    if name.startswith("dense row"):
        assert colors.max() == 7 and sorted(colors.tolist()) == [1, 2, 3, 4, 5, 6, 7]
    # a column without entries conflicts with nothing: colour 1
    assert np.all(colors[np.diff(colptr) == 0] == 1)
    # the model's checker notices a spoilt colouring
    if delta > 0:
        j = int(np.argmax([c.size for c in cm.conflicts(M, N, colptr, rowval)]))
        spoilt = colors.copy()
        spoilt[j] = colors[cm.conflicts(M, N, colptr, rowval)[j][0]]
        assert not cm.valid(M, colptr, rowval, spoilt)


def test_priority_function_is_pinned():
    # murmur3's fmix64 of j + 0x9E3779B97F4A7C15: the device source (csrc/fdjac_color.hip, color_prio), the header's text and
    # the model must not drift apart silently
    want = [0x9CA066F1A4AB2EEA, 0xE5FDC025E13EEED5, 0xF8F76353B6D877C5, 0x5FDCEF4B3D6AD6DC,
            0xE79C6FAF30EB1751, 0x6C45141841D3019F, 0x1F77F48473D16B62, 0x12B56A2136F84755]
    assert [int(v) for v in cm.prio(np.arange(8))] == want
    # restated with Python integers
    def fmix(j):
        m = (1 << 64) - 1
        x = (j + 0x9E3779B97F4A7C15) & m
        x ^= x >> 33
        x = (x * 0xFF51AFD7ED558CCD) & m
        x ^= x >> 33
        x = (x * 0xC4CEB9FE1A85EC53) & m
        return x ^ (x >> 33)
    js = [0, 1, 7, 12345, (1 << 31) - 2]
    assert [int(v) for v in cm.prio(np.array(js))] == [fmix(j) for j in js]
    # the constants as the device source and the header spell them
    src = open(os.path.join(ROOT, "finitediff.jl_amd", "csrc", "fdjac_color.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    for const in ("0x9E3779B97F4A7C15", "0xFF51AFD7ED558CCD", "0xC4CEB9FE1A85EC53"):
        assert const in src and const in hdr, const
    assert src.count("x ^= x >> 33") == 3 and hdr.count("x ^= x >> 33") == 3
    # a bijection has no ties
    assert np.unique(cm.prio(np.arange(200000))).size == 200000


def test_device_colouring_symbols_in_header_binding_shim_and_library():
    names = ("fd_color_columns_device", "fd_color_check_device")
    hdr = open(os.path.join(ROOT, "include", "fdjac.h")).read()
    shim = open(os.path.join(ROOT, "finitediff.jl_amd", "julia", "FiniteDiffMI355X.jl")).read()
    fd.lib.build()
    L = fd.lib.load()
    for name in names:
        assert re.search(r"^int %s\(fd_ctx \*ctx, int64_t M, int64_t N, const void \*colptr_dev, const void \*rowval_dev, int idx_bytes,$" % name,
                         hdr, re.M), name
        assert name in fd.lib.EXPORTS and "fd32_" + name[3:] not in fd.lib.EXPORTS        # element-type independent: no Float32 twin
        assert "ccall((:%s, libfdjac), Cint," % name in shim
        fn = getattr(L, name)
        assert len(fn.argtypes) == 10 and fn.restype is C.c_int
        # a NULL context is an argument error with a message -- no GPU is needed to learn that
        out = C.c_int64(-1)
        rc = fn(None, 3, 3, None, None, 4, 1, None, 4, C.byref(out))
        assert rc == 1 and b"NULL" in L.fd_last_error()        # FD_ERR_ARG
    assert callable(fd.matrix_colors_device) and callable(fd.check_colors_device)
    assert "matrix_colors(J::DevicePatternCSC" in shim and "check_colors(J::DevicePatternCSC" in shim
    assert L.fd_version() == 500
