"""The host path of the content fingerprints (fdjac_fingerprint3 with memkind = FD_HOST: what a plan built from host arrays records)
against the numpy model tests/fingerprint_model.py, over the case table the GPU test runs on k_fingerprint -- and the model's own
bookkeeping (pair_classes, the grid formulas) checked against a thread-by-thread run of the device loops.  No GPU."""
import numpy as np
import pytest

import fingerprint_model as M
import finitediff_jl_amd as fd


@pytest.fixture(scope="module")
def L():
    fd.lib.build()
    return fd.lib.load()


def _host_word(L, case, buf):
    """The case through the host path, reached the way the case says (i0 on the allocation, or a view of it)."""
    if case.way == "i0":
        ptr, i0 = buf.ctypes.data, case.offset
    else:
        ptr, i0 = buf[case.offset:].ctypes.data, 0
    return M.call_fingerprint3(L, None, [ptr, None, None], [case.width, 8, 8], [i0, 0, 0], [case.n, 0, 0], [case.base, 0, 0])


@pytest.mark.parametrize("kind", ["small", "gridend", "unrolled"])
def test_host_path_equals_the_model_on_the_case_table(L, kind):
    cases = [c for c in M.CASES if c.name.startswith(kind)]
    assert cases
    for case in cases:
        buf = M.case_buffer(case)
        v = M.case_values(case, buf)
        assert v.size == case.n and v.itemsize == case.width
        if case.n >= 3:
            assert set(M.EDGE32) <= set(int(x) for x in v[np.isin(v, M.EDGE32)]), case.name
        h = _host_word(L, case, buf)
        assert h == [M.fingerprint(v, case.base), 0, 0], case.name


def test_host_path_threaded_split_odd_length(L):
    # >= 2^20 pairs: host_fingerprint splits the pairs between threads; an odd length puts the sentinel partner in the last thread's range
    n = (1 << 21) + 4097
    assert (n + 1) // 2 >= 1 << 20 and n % 2 == 1
    rng = np.random.default_rng(77)
    for dt, base in ((np.int64, 1), (np.int32, 0)):
        a = rng.integers(0, 2 ** 31 - 1, size=n + 4, dtype=np.int64).astype(dt)
        a[[3, n + 2, n // 2]] = [0, 2 ** 31 - 1, -2 ** 31]
        w = a.itemsize
        h = M.call_fingerprint3(L, None, [a.ctypes.data, None, None], [w, 8, 8], [3, 0, 0], [n, 0, 0], [base, 0, 0])
        assert h == [M.fingerprint(a[3:3 + n], base), 0, 0]
        assert h[0] != M.fingerprint(a[3:2 + n], base) and h[0] != M.fingerprint(a[3:4 + n], base)      # (the length counts)


def test_host_path_three_arrays_null_and_empty_members(L):
    rng = np.random.default_rng(78)
    a32 = rng.integers(0, 2 ** 31, size=1003, dtype=np.int64).astype(np.int32)
    a64 = rng.integers(0, 2 ** 31, size=517, dtype=np.int64)
    c32 = rng.integers(0, 2 ** 31, size=64, dtype=np.int64).astype(np.int32)
    p32, p64, pc = a32.ctypes.data, a64.ctypes.data, c32.ctypes.data
    h = M.call_fingerprint3(L, None, [p32, p64, pc], [4, 8, 4], [3, 1, 0], [999, 516, 64], [1, 0, 0])
    assert h == [M.fingerprint(a32[3:1002], 1), M.fingerprint(a64[1:517]), M.fingerprint(c32)]
    # every slot in turn NULL, and with n = 0: its word is 0, the others are what they were
    for k in range(3):
        ptrs, ns = [p32, p64, pc], [999, 516, 64]
        ptrs[k] = None
        want = list(h)
        want[k] = 0
        assert M.call_fingerprint3(L, None, ptrs, [4, 8, 4], [3, 1, 0], ns, [1, 0, 0]) == want
        ptrs[k] = [p32, p64, pc][k]
        ns[k] = 0
        assert M.call_fingerprint3(L, None, ptrs, [4, 8, 4], [3, 1, 0], ns, [1, 0, 0]) == want
    assert M.call_fingerprint3(L, None, [None, None, None], [8, 8, 8], [0, 0, 0], [0, 0, 0], [0, 0, 0]) == [0, 0, 0]


def test_edge_values_and_index_width(L):
    # a function of the VALUES: 0 of a 1-based array is -1 in both widths; 2^31 - 1 and -2^31 widened to Int64 give the same word
    for vals in ([0], [0, 0], [2 ** 31 - 1, -2 ** 31, 0], [-2 ** 31, 2 ** 31 - 1], [-2 ** 31], [5, 0, 2 ** 31 - 1, 7, -2 ** 31, 0, 1]):
        for base in (0, 1):
            a32, a64 = np.array(vals, dtype=np.int32), np.array(vals, dtype=np.int64)
            h32 = M.call_fingerprint3(L, None, [a32.ctypes.data, None, None], [4, 8, 8], [0, 0, 0], [a32.size, 0, 0], [base, 0, 0])[0]
            h64 = M.call_fingerprint3(L, None, [a64.ctypes.data, None, None], [8, 8, 8], [0, 0, 0], [a64.size, 0, 0], [base, 0, 0])[0]
            assert h32 == h64 == M.fingerprint(vals, base), (vals, base)
    # the model's own arithmetic at -1: one pair (-1, sentinel) at k = 0, by hand in Python integers
    m64 = (1 << 64) - 1
    z = ((-1 & m64) + (M.SENTINEL << 32)) & m64
    z = ((z ^ (z >> 29)) * 0xBF58476D1CE4E5B9) & m64
    assert M.fingerprint([0], 1) == z ^ (z >> 32)
    # position-dependent: the pair index enters (k * K)
    assert M.fingerprint([1, 2, 3, 4]) != M.fingerprint([3, 4, 1, 2]) and M.fingerprint([1, 2]) != M.fingerprint([2, 1])


def test_pair_classes_partition_and_named_cases():
    # every case of the table: each pair has one class, the named path is there, the tail / sentinel counts are what the name says
    for case in M.CASES:
        cls = M.check_case_reaches_its_path(case, M.MI355X_CUS)
        assert cls.size == (case.n + 1) // 2
    # against the device loops run thread by thread: every pair added exactly once, in the class pair_classes gives it
    for width, offs in ((4, (0, 1, 2, 3)), (8, (0, 1))):
        for off in offs:
            for n in M.SMALL_LENGTHS + (4096 + 3, 4096 + 256 * 8 * 2 + 5):
                for stride in (2, 256, 512):
                    if stride == 2 and n > 600:
                        continue
                    got, hits = M.simulate_classes(n, width, off * width, stride)
                    assert np.all(hits == 1), (n, width, off, stride)
                    assert np.array_equal(got, M.pair_classes(n, width, off * width, stride)), (n, width, off, stride)
    # the lengths the issue names
    q = lambda n: M.pair_classes(n, 4, 0, 256)
    assert [M.class_name(c) for c in q(4)] == ["quads", "quads"]
    assert all((c & 7) == M.VEC for n in (1, 2, 3) for c in q(n))
    assert [M.class_name(c) for c in q(5)][-1] == "quad_tail+odd_last" and [M.class_name(c) for c in q(6)][-1] == "quad_tail"
    assert [M.class_name(c) for c in q(7)][-2:] == ["quad_tail", "quad_tail+odd_last"]
    assert M.class_name(M.pair_classes(8, 4, 0, 256)[-1]) == "quads"
    u = M.pair_classes(4 * 256 * 9, 4, 0, 256)                      # 9 quads per thread: 8 unrolled + 1
    assert int(np.sum(u == (M.QUADS | M.UNROLLED))) == 2 * 256 * 8 and int(np.sum(u == M.QUADS)) == 2 * 256


def test_grid_formulas():
    cus = M.MI355X_CUS
    assert [M.k_fingerprint_grid(n, cus) for n in (1, 256, 257, 256 * 511, 256 * 511 + 1, 256 * 512 + 1, 10 ** 9)] == [1, 1, 2, 511, 512, 512, 512]
    below, at, above = (c for c in M.grid_end_cases(cus) if c.width == 4 and c.offset == 0 and c.n % 256 == 1)
    assert [(c.n + 255) // 256 for c in (below, at, above)] == [2 * cus - 1, 2 * cus, 2 * cus + 1]
    assert [M.k_fingerprint_grid(c.n, cus) for c in (below, at, above)] == [2 * cus - 1, 2 * cus, 2 * cus]
    # the fused launch: one member -> its share is the whole budget + 1; left-out members get no workgroup
    assert M.fused_grids((0, 0, 2048 * 33), (8, 8, 4), cus) == ((0, 0, 33), (0, 0, 4 * cus + 1), 33)
    assert M.fused_grids((0, 0, 1), (8, 8, 8), cus).g == (0, 0, 1)
    big = M.fused_grids((0, 0, 2048 * (4 * cus + 1) * 8 + 3), (8, 8, 4), cus)
    assert big.g == (0, 0, 4 * cus + 1) == big.share
    # by bytes: rowval 12 x colptr in Int64, Int32 colours
    N = 20480
    f = M.fused_grids((N + 1, 12 * N, N), (8, 8, 4), cus)
    assert f.g == (11, 120, 10) and f.total == 141 and all(s > g for s, g in zip(f.share, f.g))
    assert sum(f.share) <= 4 * cus + 3                             # what fdjac_fingerprint3_check_words leaves room for
