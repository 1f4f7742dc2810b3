"""Host model of the content fingerprints (csrc/fdjac_match.hip): the value, which device code path sums which pair, and the grids
the two launchers choose -- pure numpy / ctypes, no GPU.

    F(a) = sum_k mix(v_2k + (v_2k+1 << 32) + k * K)   (mod 2^64;  v_i = a[i0 + i] - base, widened to 64 bits;
                                                        a missing last partner counts as 0x7fffffff)
    mix(z) = (z ^ (z >> 29)) * C, then ^ (>> 32)

`fingerprint` is the definition (the header comment of the file and its host path).  `pair_classes` restates the branch conditions of
fp_pairs_any / fp_quads32 / fp_pairs, `k_fingerprint_grid` / `fused_grids` the grid formulas of fdjac_fingerprint3 /
fdjac_fingerprint3_check: the tests use them to ASSERT that a case reaches the path / grid it is named for and to choose where to edit.
The case table of the absolute-value tests (tests/test_fingerprint_model_cpu.py on the host path, tests/test_gpu_fingerprint.py on
k_fingerprint) lives here as well."""
import collections
import ctypes as C

import numpy as np

K = 0xD6E8FEB86659FD93
SENTINEL = 0x7fffffff
FD_HOST, FD_DEVICE = 0, 1
MI355X_CUS = 256


def fingerprint(values, base=0):
    """F(values - base): uint64 arithmetic that wraps; every value is widened to 64 bits, then the base is subtracted (a 0 of a 1-based
    array is -1 = 2^64 - 1 in either index width)."""
    with np.errstate(over="ignore"):
        v = (np.asarray(values, dtype=np.int64) - base).astype(np.uint64)
        if v.size % 2:
            v = np.concatenate([v, np.array([SENTINEL], dtype=np.uint64)])
        v0, v1 = v[0::2], v[1::2]
        k = np.arange(v0.size, dtype=np.uint64)
        z = v0 + (v1 << np.uint64(32)) + k * np.uint64(K)
        z = (z ^ (z >> np.uint64(29))) * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(32))
        return int(np.sum(z, dtype=np.uint64))


# ---- which device path sums which pair ----------------------------------------------------------------------------------------------
# the class of a pair = its path, | UNROLLED when the U = 8 loop of that path adds it (otherwise its remainder loop; the quad tail has
# no loop), | ODD_LAST for the pair of the last odd element (partner = the sentinel, in whichever path adds it)
QUADS, QUAD_TAIL, VEC, SCALAR = 0, 1, 2, 3
UNROLLED, ODD_LAST = 8, 16
PATH_NAMES = {QUADS: "quads", QUAD_TAIL: "quad_tail", VEC: "vec", SCALAR: "scalar"}
U = 8


def class_name(c):
    c = int(c)
    return PATH_NAMES[c & 7] + ("+unrolled" if c & UNROLLED else "") + ("+odd_last" if c & ODD_LAST else "")


def _strided_unrolled(count, stride):
    """Items 0 .. count-1 dealt to `stride` threads (thread t: t, t + stride, ...), each thread taking U at a time while U remain
    (`for (; k + (U - 1) * stride < count; k += U * stride)`): which items does an unrolled iteration take?"""
    idx = np.arange(count, dtype=np.int64)
    t, j = idx % stride, idx // stride
    per_thread = (count - t + stride - 1) // stride
    return j < U * (per_thread // U)


def pair_classes(n, width_bytes, start_misalign_bytes, stride_threads):
    """Class of every pair 0 .. ceil(n / 2) - 1 of a range of `n` elements of `width_bytes` whose first element lies
    `start_misalign_bytes` past a 16-byte boundary, summed by `stride_threads` threads (grid * 256)."""
    n, w, mis, stride = int(n), int(width_bytes), int(start_misalign_bytes) % 16, int(stride_threads)
    assert w in (4, 8) and mis % w == 0 and stride >= 2 and n >= 1
    npairs = (n + 1) // 2
    cls = np.empty(npairs, dtype=np.int8)
    if w == 4 and mis == 0 and n >= 4:                         # fp_pairs_any: fp_quads32 + the pairs of the last n mod 4 elements
        nquads = n // 4
        cls[:2 * nquads] = QUADS | np.repeat(_strided_unrolled(nquads, stride), 2) * UNROLLED
        cls[2 * nquads:] = QUAD_TAIL                           # (threads 0 / 1 of the grid: stride >= 2)
    else:                                                       # fp_pairs<IT, VEC>: VEC = the start is aligned to two elements
        path = VEC if mis % (2 * w) == 0 else SCALAR
        cls[:] = path | _strided_unrolled(npairs, stride) * UNROLLED
    if n % 2:
        cls[-1] |= ODD_LAST
    return cls


def simulate_classes(n, width_bytes, start_misalign_bytes, stride_threads):
    """The same by running the device loops thread by thread (small n only): returns (classes, times each pair was added)."""
    n, w, mis, stride = int(n), int(width_bytes), int(start_misalign_bytes) % 16, int(stride_threads)
    npairs = (n + 1) // 2
    cls, hits = np.full(npairs, -1, dtype=np.int8), np.zeros(npairs, dtype=np.int64)

    def add(k, c):
        cls[k] = c | (ODD_LAST if 2 * k + 1 >= n else 0)
        hits[k] += 1

    def loops(count, k0, body):
        k = k0
        while k + (U - 1) * stride < count:
            for u in range(U):
                body(k + u * stride, UNROLLED)
            k += U * stride
        while k < count:
            body(k, 0)
            k += stride

    quads = w == 4 and mis == 0 and n >= 4
    for k0 in range(min(stride, max(npairs, 2))):
        if quads:
            def body(q, un):
                add(2 * q, QUADS | un)
                add(2 * q + 1, QUADS | un)
            loops(n // 4, k0, body)
            kt = 2 * (n // 4)
            if k0 < npairs - kt:
                add(kt + k0, QUAD_TAIL)
        else:
            path = VEC if mis % (2 * w) == 0 else SCALAR
            loops(npairs, k0, lambda k, un: add(k, path | un))
    return cls, hits


def pick(classes, c, where="middle"):
    """A pair index of class `c`."""
    idx = np.flatnonzero(classes == c)
    assert idx.size, class_name(c)
    return int(idx[{"first": 0, "middle": idx.size // 2, "last": -1}[where]])


# ---- the launchers' grids -----------------------------------------------------------------------------------------------------------
def k_fingerprint_grid(n, cus):
    """Workgroups of k_fingerprint over `n` elements (fdjac_fingerprint3)."""
    return min((int(n) + 255) // 256, 2 * int(cus))


FusedGrids = collections.namedtuple("FusedGrids", "g share total")


def fused_grids(n3, bytes3, cus, per_cu=4):
    """Workgroups per array of k_fingerprint3_check (fdjac_fingerprint3_check): a few per CU in all, shared out by bytes (+ 1), at most
    one per 2048 elements, at least one for a member that is compared; n = 0 leaves a member out."""
    all_bytes = 0.0
    for n, b in zip(n3, bytes3):
        all_bytes += float(n) * b if n > 0 else 0.0
    g, share = [], []
    for n, b in zip(n3, bytes3):
        if n > 0:
            s = int(float(cus) * per_cu * (float(n) * b / all_bytes)) + 1
            share.append(s)
            g.append(max(1, min((int(n) + 2047) // 2048, s)))
        else:
            share.append(0)
            g.append(0)
    return FusedGrids(tuple(g), tuple(share), sum(g))


# ---- the library call ---------------------------------------------------------------------------------------------------------------
def call_fingerprint3(L, ctx_handle, ptrs, widths, i0, n, base, memkind=FD_HOST, acc_ptr=None):
    """fdjac_fingerprint3 over up to three arrays given by address (None = NULL): the three words."""
    a = (C.c_void_p * 3)(*[C.c_void_p(p) if p else None for p in ptrs])
    out = (C.c_uint64 * 3)(1, 1, 1)
    rc = L.fdjac_fingerprint3(ctx_handle, a, (C.c_int * 3)(*widths), (C.c_int64 * 3)(*i0), (C.c_int64 * 3)(*n), (C.c_int64 * 3)(*base),
                              C.c_int(memkind), C.c_void_p(acc_ptr) if acc_ptr else None, out)
    assert rc == 0, rc
    return [int(v) for v in out]


# ---- the case table of the absolute-value tests -------------------------------------------------------------------------------------
# a case: `n` elements of `width` bytes, `base`-based, starting `offset` elements past a 16-byte aligned allocation -- reached as
# i0 = offset on the aligned pointer (way "i0") or as a view t[offset:] with i0 = 0 (way "view"); `path` is the path the case is
# NAMED for (written down by hand per width / offset, not computed from the alignment), `expect` further classes it must contain.
Case = collections.namedtuple("Case", "name width base offset way n path expect seed")
SMALL_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 511, 513, 2047, 2048, 2049)
NAMED_PATH = {(4, 0): "quads", (4, 1): "scalar", (4, 2): "vec", (4, 3): "scalar", (8, 0): "vec", (8, 1): "scalar"}
EDGE32 = (0, 2 ** 31 - 1, -2 ** 31)


def small_cases():
    out = []
    for width, offsets in ((4, (0, 1, 2, 3)), (8, (0, 1))):
        for base in (0, 1):
            for off in offsets:
                for way in ("i0", "view"):
                    for n in SMALL_LENGTHS:
                        path = NAMED_PATH[(width, off)]
                        if path == "quads" and n < 4:
                            path = "vec"                                   # 1 .. 3 elements fall to the pairs
                        out.append(Case("small-w%d-b%d-o%d-%s-n%d" % (width, base, off, way, n), width, base, off, way, n, path, (),
                                        len(out)))
    return out


def grid_end_cases(cus):
    """ceil(n / 256) = 2 CUs - 1, 2 CUs, 2 CUs + 1: the grid of k_fingerprint below, at and above its cap."""
    out = []
    for width, off in ((4, 0), (4, 1), (8, 0)):
        for blocks in (2 * cus - 1, 2 * cus, 2 * cus + 1):
            for n in (256 * (blocks - 1) + 1, 256 * blocks - 1):
                out.append(Case("gridend-w%d-o%d-blocks%d-n%d" % (width, off, blocks, n), width, 1, off, "i0", n,
                                NAMED_PATH[(width, off)], (), 7000 + len(out)))
    return out


def unrolled_cases(cus):
    """Long enough for U = 8 iterations per thread of the capped grid, with a factor 2 of margin: S = 2 CUs * 256 threads, 16 S quads
    (Int32 on the boundary) or pairs, + r elements.  At exactly 16 S every thread runs two unrolled iterations and NO remainder
    iteration (r = 1 off the quad path gives thread 0 one), so each group has a companion 384 quads / pairs longer: the first 384
    threads -- more than one workgroup -- then run the remainder loop once as well."""
    s16 = 16 * (2 * cus * 256)
    out = []
    for width, off, per, rs in ((4, 0, 4, (0, 1, 2, 3)), (4, 1, 2, (0, 1)), (4, 2, 2, (0, 1)), (8, 0, 2, (0, 1)), (8, 1, 2, (0, 1))):
        for extra in (0, 384):
            for r in (rs if extra == 0 else rs[-1:]):
                n = per * (s16 + extra) + r
                expect = ("unrolled", "remainder") if extra or (per == 2 and r == 1) else ("unrolled", "no remainder")
                out.append(Case("unrolled-w%d-o%d-x%d-r%d" % (width, off, extra, r), width, r % 2, off, "i0" if r % 2 == 0 else "view", n,
                                NAMED_PATH[(width, off)], expect, 9000 + len(out)))
    return out


def case_table(cus=MI355X_CUS):
    return small_cases() + grid_end_cases(cus) + unrolled_cases(cus)


CASES = case_table()


def case_buffer(case, pad=5):
    """The case's allocation (numpy): `offset` guard elements, the n values, `pad` guard elements.  Values: random 31-bit ones, the
    edges 0 / 2^31 - 1 / -2^31 at the first, the last and three random places (as far as the length goes)."""
    rng = np.random.default_rng(40000 + case.seed)
    dt = np.int32 if case.width == 4 else np.int64
    buf = rng.integers(0, 2 ** 31, size=case.offset + case.n + pad, dtype=np.int64).astype(dt)
    v = buf[case.offset:case.offset + case.n]
    spots = np.unique(np.concatenate([[0, case.n // 2, case.n - 1], rng.integers(0, case.n, size=3)]))
    for j, s in enumerate(rng.permutation(spots)):
        v[s] = EDGE32[j % 3]
    return buf


def case_values(case, buf):
    return buf[case.offset:case.offset + case.n]


def case_classes(case, cus):
    """pair_classes of the case under k_fingerprint's grid (the allocation is 16-byte aligned)."""
    return pair_classes(case.n, case.width, case.offset * case.width % 16, 256 * k_fingerprint_grid(case.n, cus))


def check_case_reaches_its_path(case, cus):
    """The assertions every named case makes about itself (shared by the CPU self-check and the GPU test)."""
    cls = case_classes(case, cus)
    paths = set(PATH_NAMES[int(c) & 7] for c in np.unique(cls))
    assert case.path in paths, (case.name, paths)
    if case.path != "quads":
        assert paths == {case.path}, (case.name, paths)                   # no quad path off the 16-byte boundary / below 4 elements
    else:
        tail = int(np.sum((cls & 7) == QUAD_TAIL))
        assert tail == (case.n % 4 + 1) // 2 and paths == ({"quads", "quad_tail"} if tail else {"quads"}), (case.name, paths)
    assert bool(cls[-1] & ODD_LAST) == bool(case.n % 2) and not np.any(cls[:-1] & ODD_LAST), case.name
    own = (cls & 7) == {"quads": QUADS, "vec": VEC, "scalar": SCALAR}[case.path]
    if "unrolled" in case.expect:
        assert np.any(own & ((cls & UNROLLED) != 0)), case.name
    if "remainder" in case.expect:
        assert np.any(own & ((cls & UNROLLED) == 0)), case.name
    if "no remainder" in case.expect:
        assert not np.any(own & ((cls & UNROLLED) == 0)), case.name
    return cls
