"""The device side of the content check (csrc/fdjac_match.hip) against the host model tests/fingerprint_model.py: the absolute value
of k_fingerprint on every summing path (quads unrolled / remainder / tail, one vector load per pair, scalar, the last odd element), at
every start alignment -- as i0 and as a tensor view -- around the grid's cap and inside the unrolled loops; the blocking verdict
(fd_plan_matches) and the deferred one (fd_plan_matches_async: k_fingerprint3_check, its shares, slots and self-resetting tickets) for
edits at the places the paths hand over to each other.  Every assertion is integer equality or a boolean verdict, and every named case
asserts through pair_classes / k_fingerprint_grid / fused_grids that it reaches the path or grid it is named for.

A test that expects FD_ERR_STALE drains the context's sticky word: the synchronize() that raises clears it, a second one must not
raise."""
import numpy as np
import pytest

import fingerprint_model as M
import finitediff_jl_amd as fd
from finitediff_jl_amd import patterns as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FD_ERR_STALE = 9


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count      # what fd_ctx holds (num_cus)


@pytest.fixture(scope="module")
def ctx():
    return fd.Context.default()


@pytest.fixture(scope="module")
def acc():
    return torch.zeros(3, dtype=torch.int64, device="cuda")              # the launcher's three device words


@pytest.fixture(autouse=True)
def _leave_no_verdict_behind(ctx):
    yield
    try:                                                                   # (a FAILED test may not have drained the context's word)
        ctx.synchronize()
    except fd.lib.FdError:
        pass


def _dev(a):
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    assert t.data_ptr() % 16 == 0
    return t


# =====================================================================================================================================
# a. the absolute value of k_fingerprint
# =====================================================================================================================================
def _device_word(ctx, acc, case, t):
    """fdjac_fingerprint3 on the device copy `t` of the case's allocation, reached the way the case says."""
    if case.way == "i0":
        ptr, i0 = t.data_ptr(), case.offset
    else:
        v = t[case.offset:]
        assert v.storage_offset() == case.offset and v.is_contiguous()
        ptr, i0 = v.data_ptr(), 0
    assert (ptr + i0 * case.width) % 16 == case.offset * case.width % 16      # the alignment case_classes assumes
    acc.fill_(-1)                                                               # (the launcher zeroes its accumulators itself)
    return M.call_fingerprint3(ctx.L, ctx.handle, [ptr, None, None], [case.width, 8, 8], [i0, 0, 0], [case.n, 0, 0], [case.base, 0, 0],
                               M.FD_DEVICE, acc.data_ptr())


def _check_case(ctx, acc, cus, case):
    M.check_case_reaches_its_path(case, cus)
    buf = M.case_buffer(case)
    want = M.fingerprint(M.case_values(case, buf), case.base)
    got = _device_word(ctx, acc, case, _dev(buf))
    assert got == [want, 0, 0], (case.name, [M.class_name(c) for c in np.unique(M.case_classes(case, cus))])


@pytest.mark.parametrize("way", ["i0", "view"])
@pytest.mark.parametrize("width,offset", [(4, 0), (4, 1), (4, 2), (4, 3), (8, 0), (8, 1)])
def test_k_fingerprint_value_small_lengths(ctx, acc, cus, width, offset, way):
    cases = [c for c in M.small_cases() if (c.width, c.offset, c.way) == (width, offset, way)]
    assert len(cases) == 2 * len(M.SMALL_LENGTHS) and {c.base for c in cases} == {0, 1}
    for case in cases:
        _check_case(ctx, acc, cus, case)


def test_k_fingerprint_value_around_the_grid_cap(ctx, acc, cus):
    cases = M.grid_end_cases(cus)
    for width, off in ((4, 0), (4, 1), (8, 0)):
        grp = [c for c in cases if (c.width, c.offset) == (width, off)]
        assert sorted({(c.n + 255) // 256 for c in grp}) == [2 * cus - 1, 2 * cus, 2 * cus + 1]
        assert sorted({M.k_fingerprint_grid(c.n, cus) for c in grp}) == [2 * cus - 1, 2 * cus]       # below the cap, and capped twice
    for case in cases:
        _check_case(ctx, acc, cus, case)


@pytest.mark.parametrize("name", [c.name for c in M.unrolled_cases(M.MI355X_CUS)])
def test_k_fingerprint_value_unrolled_loops(ctx, acc, cus, name):
    case, = [c for c in M.unrolled_cases(cus) if c.name == name]
    assert M.k_fingerprint_grid(case.n, cus) == 2 * cus and "unrolled" in case.expect
    _check_case(ctx, acc, cus, case)


def test_k_fingerprint_three_arrays_in_one_call(ctx, acc):
    rng = np.random.default_rng(79)
    h32 = rng.integers(0, 2 ** 31, size=1003, dtype=np.int64).astype(np.int32)
    h64 = rng.integers(0, 2 ** 31, size=517, dtype=np.int64)
    hc = rng.integers(0, 2 ** 31, size=70, dtype=np.int64).astype(np.int32)
    h32[[3, 500, 1001]] = M.EDGE32
    h64[[1, 200, 516]] = M.EDGE32
    d32, d64, dc = _dev(h32), _dev(h64), _dev(hc)
    p32, p64, pc = d32.data_ptr(), d64.data_ptr(), dc[2:].data_ptr()         # (the colours through a view: 8 bytes past the boundary)
    args = ([4, 8, 4], [3, 1, 0], [999, 516, 68], [1, 0, 0])
    want = [M.fingerprint(h32[3:1002], 1), M.fingerprint(h64[1:517]), M.fingerprint(hc[2:])]

    def run(ptrs, ns):
        acc.fill_(-1)
        return M.call_fingerprint3(ctx.L, ctx.handle, ptrs, args[0], args[1], ns, args[3], M.FD_DEVICE, acc.data_ptr())
    assert run([p32, p64, pc], args[2]) == want
    for k in range(3):                                                          # every slot in turn NULL, and with n = 0
        ptrs, ns, w = [p32, p64, pc], list(args[2]), list(want)
        ptrs[k], w[k] = None, 0
        assert run(ptrs, ns) == w
        ptrs[k], ns[k] = [p32, p64, pc][k], 0
        assert run(ptrs, ns) == w
    assert run([None, None, None], [0, 0, 0]) == [0, 0, 0]


# =====================================================================================================================================
# b. / c. the verdicts through the public API
# =====================================================================================================================================
NB = 4099
WINDOWS = [None, (1000, 3001), (1001, 3003), (1002, 3006), (1003, 3010)]


def _csc(N, per):
    """`per` entries in every column (rows j .. j + per - 1, shifted to stay inside), 1-based Int64; colours of period 2 per."""
    start = np.minimum(np.arange(N, dtype=np.int64), N - per)
    cp = 1 + per * np.arange(N + 1, dtype=np.int64)
    rv = (start[:, None] + np.arange(per, dtype=np.int64)[None, :]).ravel() + 1
    return cp, rv, P.cyclic_colors(N, 2 * per)


def _device_copies(host, npdt, view):
    """Device copies of the arrays in one width; view: one element more, sliced -- same content, start one element off."""
    out = []
    for a in host:
        if view:
            t = _dev(np.concatenate([[12345], a]).astype(npdt))[1:]
            assert t.data_ptr() % 16 == t.element_size() and t.is_contiguous()
        else:
            t = _dev(a.astype(npdt))
        out.append(t)
    return out


def _ranges(cp, N, window):
    """(first element, length) of what a CSC plan fingerprints: colptr[a .. b], rowval[cp[a] - 1 .. cp[b] - 1), every colour."""
    a, b = window if window else (0, N)
    return [(a, b - a + 1), (int(cp[a]) - 1, int(cp[b] - cp[a])), (0, N)]


def _classes(arrs, ranges, strides):
    out = []
    for t, (i0, n), s in zip(arrs, ranges, strides):
        out.append(M.pair_classes(n, t.element_size(), (t.data_ptr() + i0 * t.element_size()) % 16, s))
    return out


def _edit_table(arrs, ranges, classes):
    """(label, array, element) -- inside: what the plan compares; outside: the neighbours of its ranges."""
    (a0, an), (b0, bn), (_c0, cn) = ranges
    inside = [("colptr first", 0, a0), ("colptr last", 0, a0 + an - 1), ("rowval first", 1, b0), ("rowval last", 1, b0 + bn - 1)]
    inside += [("colour %d from the end" % q, 2, cn - q) for q in (1, 2, 3, 4)]
    for k, ((i0, n), cls) in enumerate(zip(ranges, classes)):
        for c in np.unique(cls):
            kp = M.pick(cls, c)
            inside.append(("%s of array %d" % (M.class_name(c), k), k, i0 + min(2 * kp + kp % 2, n - 1)))      # either partner
    outside = [("before colptr", 0, a0 - 1), ("after colptr", 0, a0 + an), ("before rowval", 1, b0 - 1), ("after rowval", 1, b0 + bn)]
    outside = [(lab, k, j) for lab, k, j in outside if 0 <= j < arrs[k].numel()]
    return inside, outside


def _csc_plan_maker(builder, cp, rv, cv, N, window):
    kw = {"col_window": window} if window else {}
    if builder == "host":
        pat = fd.SparseMatrixCSC(N, N, cp, rv, None)
        return lambda: fd.make_plan(pat, pat, cv, "forward", fingerprint=True, **kw)
    src = _device_copies((cp, rv, cv), np.int32, False)
    return lambda: fd.make_plan_csc_device(N, N, src[0], src[1], src[2], "forward", fingerprint=True, **kw)


def _paths_seen(classes):
    return {M.class_name(c) for c in np.unique(classes)}


def _assert_paths_seen(seen, width, view):
    # windows with a mod 4 = 0 .. 3 (and the view's extra element) put the starts of colptr and rowval at every alignment; the 4099
    # colours end in a quad tail of two pairs when they start on the boundary
    base = {s.split("+")[0] for s in seen}
    assert ({"quads", "vec", "scalar"} if width == 4 else {"vec", "scalar"}) <= base, seen
    assert any(s.endswith("odd_last") for s in seen), seen
    if width == 4 and not view:
        assert {"quad_tail", "quad_tail+odd_last"} <= seen, seen


def _assert_windows_cover_alignments(cp):
    ws = [w for w in WINDOWS if w]
    assert sorted(a % 4 for a, _b in ws) == [0, 1, 2, 3] and sorted((int(cp[a]) - 1) % 4 for a, _b in ws) == [0, 1, 2, 3]


VARIANTS = [(np.int32, False), (np.int32, True), (np.int64, False), (np.int64, True)]


@pytest.mark.parametrize("npdt,view", VARIANTS)
@pytest.mark.parametrize("builder", ["host", "device"])
def test_blocking_verdict_at_every_alignment_and_edit(cus, builder, npdt, view):
    cp, rv, cv = _csc(NB, 3)
    _assert_windows_cover_alignments(cp)
    seen = set()
    for window in WINDOWS:
        plan = _csc_plan_maker(builder, cp, rv, cv, NB, window)()
        arrs = _device_copies((cp, rv, cv), npdt, view)
        ranges = _ranges(cp, NB, window)
        classes = _classes(arrs, ranges, [256 * M.k_fingerprint_grid(n, cus) for _i0, n in ranges])
        seen |= _paths_seen(np.concatenate(classes))
        inside, outside = _edit_table(arrs, ranges, classes)
        assert len(outside) == (4 if window else 0)
        assert plan.matches(*arrs) is True
        for lab, k, j in inside:
            arrs[k][j] += 1
            assert plan.matches(*arrs) is False, (window, lab, j)
            arrs[k][j] -= 1
        for lab, k, j in outside:
            arrs[k][j] += 1
            assert plan.matches(*arrs) is True, (window, lab, j)
            arrs[k][j] -= 1
        assert plan.matches(*arrs) is True
    _assert_paths_seen(seen, np.dtype(npdt).itemsize, view)


def _stale_after(ctx, plan, arrs, expect, what):
    """One deferred check: its verdict after synchronize(), and the context's word drained."""
    plan.matches(*arrs, deferred=True)
    if expect:
        with pytest.raises(fd.lib.FdError) as e:
            ctx.synchronize()
        assert e.value.code == FD_ERR_STALE and plan.stale(), what
        ctx.synchronize()                                                       # cleared by the one that raised
    else:
        ctx.synchronize()
        assert not plan.stale(), what


@pytest.mark.parametrize("npdt,view", VARIANTS)
@pytest.mark.parametrize("builder", ["host", "device"])
def test_deferred_verdict_at_every_alignment_and_edit(ctx, cus, builder, npdt, view):
    cp, rv, cv = _csc(NB, 3)
    _assert_windows_cover_alignments(cp)
    w = np.dtype(npdt).itemsize
    seen = set()
    for window in WINDOWS:
        make = _csc_plan_maker(builder, cp, rv, cv, NB, window)
        arrs = _device_copies((cp, rv, cv), npdt, view)
        ranges = _ranges(cp, NB, window)
        grids = M.fused_grids([n for _i0, n in ranges], [w, w, w], cus)
        assert all(g >= 1 for g in grids.g) and grids.total == sum(-(-n // 2048) for _i0, n in ranges)      # (small: below every share)
        classes = _classes(arrs, ranges, [256 * g for g in grids.g])
        seen |= _paths_seen(np.concatenate(classes))
        inside, outside = _edit_table(arrs, ranges, classes)
        assert len(outside) == (4 if window else 0)
        clean = make()
        _stale_after(ctx, clean, arrs, False, (window, "clean"))
        for lab, k, j in outside:
            arrs[k][j] += 1
            _stale_after(ctx, clean, arrs, False, (window, lab, j))
            arrs[k][j] -= 1
        for lab, k, j in inside:
            plan = make()                                                       # (stale is sticky: a plan per edit)
            arrs[k][j] += 1
            _stale_after(ctx, plan, arrs, True, (window, lab, j))
            arrs[k][j] -= 1
        _stale_after(ctx, clean, arrs, False, (window, "restored"))
    _assert_paths_seen(seen, w, view)


# ---- grid sizes and tickets: colour-only checks on structural plans, grid = ceil(N / 2048) ---------------------------------------------
def _tri_plan(N, colors):
    d = torch.empty(N, dtype=torch.float64, device="cuda")                     # (only the size of a structural plan's J matters)
    tri = fd.Tridiagonal(d[:N - 1], d, d[:N - 1])
    return fd.make_plan(tri, tri, colors, "forward", fingerprint=True)


def _first_element_of_thread(n, width, misalign, k0):
    """An element thread k0 of the sub-grid adds in its first iteration: quad k0 on the quad path, pair k0 otherwise."""
    j = 4 * k0 if (width == 4 and misalign == 0 and n >= 4 and k0 < n // 4) else 2 * k0
    assert j < n
    return j


@pytest.mark.parametrize("grid", [1, 2, 31, 32, 33, 63, 64, 65, 97])
def test_deferred_verdict_grid_sizes_and_ticket_reset(ctx, cus, grid):
    for N in (2048 * grid, 2048 * (grid - 1) + 1):
        colors = P.cyclic_colors(N, 3)
        for tdt in (torch.int32, torch.int64):
            dcv = torch.as_tensor(colors, device="cuda").to(tdt)
            w = dcv.element_size()
            assert dcv.data_ptr() % 16 == 0
            assert M.fused_grids((0, 0, N), (8, 8, w), cus).g == (0, 0, grid)
            plan = _tri_plan(N, colors)
            for rep in range(3):                                                # the tickets must have reset themselves
                _stale_after(ctx, plan, (None, None, dcv), False, (N, w, "clean", rep))
            for lab, j in (("last colour", N - 1), ("first thread of the last workgroup", _first_element_of_thread(N, w, 0, 256 * (grid - 1)))):
                plan = _tri_plan(N, colors)
                dcv[j] += 1
                _stale_after(ctx, plan, (None, None, dcv), True, (N, w, lab, j))
                dcv[j] -= 1


@pytest.mark.parametrize("grid", [1, 2, 31, 32, 33, 63, 64, 65, 97])
def test_deferred_verdict_tickets_leave_no_residue_for_another_grid(ctx, cus, grid):
    # The tickets belong to the plan, not to a grid: a window plan compares few columns and every colour, so its checks run on
    # different grids -- the colours on `grid` workgroups (clean), then colptr alone on one workgroup, or colptr + rowval on two, with
    # an edit.  A ticket that the colours' launch did not return to 0 keeps that later verdict from ever being raised.
    # (What this does NOT pin down is a group that counts too FEW arrivals, in_group = grid / G for one: the workgroups of a launch
    # arrive within the round trip of one atomic, so the late arrival's increment lands before the early winner's reset and no residue
    # is left, and the slots it would have missed are written by the time the early verdict reads them.  Measured: that mutation
    # passes this file.  Only a count that is too HIGH is caught with certainty -- by every case that expects a verdict.)
    N = 2048 * grid
    cp, rv, cv = _csc(N, 3)
    window = (100, 600)
    pat = fd.SparseMatrixCSC(N, N, cp, rv, None)
    make = lambda: fd.make_plan(pat, pat, cv, "forward", fingerprint=True, col_window=window)
    dcp, drv, dcv = _device_copies((cp, rv, cv), np.int32, False)
    (a0, an), (b0, bn), _c = _ranges(cp, N, window)
    assert M.fused_grids((0, 0, N), (4, 4, 4), cus).g == (0, 0, grid)
    assert M.fused_grids((an, 0, 0), (4, 4, 4), cus).g == (1, 0, 0) and M.fused_grids((an, bn, 0), (4, 4, 4), cus).g == (1, 1, 0)
    plan = make()
    _stale_after(ctx, plan, (None, None, dcv), False, "colours, clean")
    dcp[a0 + an - 1] += 1
    _stale_after(ctx, plan, (dcp, None, None), True, "colptr alone, edited, after the colours' grid")
    dcp[a0 + an - 1] -= 1
    plan = make()
    for rep in range(2):
        _stale_after(ctx, plan, (None, None, dcv), False, ("colours, clean", rep))
    _stale_after(ctx, plan, (dcp, drv, None), False, "colptr + rowval, clean")
    _stale_after(ctx, plan, (None, None, dcv), False, "colours, clean again")
    drv[b0 + bn - 1] += 1
    _stale_after(ctx, plan, (dcp, drv, None), True, "colptr + rowval, edited, after the colours' grid")
    drv[b0 + bn - 1] -= 1


def test_deferred_verdict_three_arrays_of_very_unequal_sizes(ctx, cus):
    # rowval 12 x colptr, Int64 indices, Int32 colours: the shares by bytes, three different sub-grids, the slot -> array assignment
    N = 20480
    cp, rv, cv = _csc(N, 12)
    pat = fd.SparseMatrixCSC(N, N, cp, rv, None)
    make = lambda: fd.make_plan(pat, pat, cv, "forward", fingerprint=True)
    arrs = [_dev(cp), _dev(rv), _dev(cv.astype(np.int32))]
    grids = M.fused_grids((N + 1, rv.size, N), (8, 8, 4), cus)
    assert rv.size == 12 * N and len(set(grids.g)) == 3 and min(grids.g) > 1 and grids.g[0] == (N + 1 + 2047) // 2048
    _stale_after(ctx, make(), arrs, False, "clean")
    for lab, k, j in (("last colptr", 0, N), ("last rowval", 1, rv.size - 1), ("last colour", 2, N - 1),
                      ("first rowval: workgroup g[0] = %d" % grids.g[0], 1, 0)):
        plan = make()
        arrs[k][j] += 1
        _stale_after(ctx, plan, arrs, True, lab)
        arrs[k][j] -= 1


def test_deferred_verdict_members_left_out(ctx, cus):
    cp, rv, cv = _csc(NB, 3)
    pat = fd.SparseMatrixCSC(NB, NB, cp, rv, None)
    make = lambda: fd.make_plan(pat, pat, cv, "forward", fingerprint=True)
    dcp, drv, dcv = _device_copies((cp, rv, cv), np.int32, False)
    mid = {0: NB // 2, 1: rv.size // 2, 2: NB // 3}
    full = (dcp, drv, dcv)
    for name, passed, compared in (("colorvec only", (None, None, dcv), (2,)), ("colptr and rowval", (dcp, drv, None), (0, 1)),
                                   ("rowval only", (None, drv, None), (1,))):
        ns = [t.numel() if t is not None else 0 for t in passed]
        ns[1] = rv.size if passed[1] is not None else 0
        g = M.fused_grids(ns, (4, 4, 4), cus).g
        assert [x > 0 for x in g] == [k in compared for k in range(3)], name
        clean = make()
        _stale_after(ctx, clean, passed, False, (name, "clean"))
        for k in range(3):
            full[k][mid[k]] += 1
            if k in compared:
                _stale_after(ctx, make(), passed, True, (name, "edit in member", k))
            else:
                _stale_after(ctx, clean, passed, False, (name, "edit in a member that is not compared", k))
            full[k][mid[k]] -= 1
        _stale_after(ctx, clean, passed, False, (name, "restored"))


@pytest.mark.parametrize("tdt", [torch.int32, torch.int64])
def test_deferred_verdict_unrolled_loop_of_the_fused_kernel(ctx, cus, tdt):
    # share is the cap: 4 CUs + 1 workgroups, 16 quads (Int32) or 32 pairs (Int64) per thread and 3 elements more.  Four plans per
    # width: clean (twice), an edit in the unrolled loop, one outside it, the last element.  Int32: every thread runs exactly two
    # unrolled iterations and the quad remainder loop is empty -- the edit outside the loop goes to the quad tail; Int64: four unrolled
    # iterations, and the remainder loop has the two pairs of threads 0 and 1.
    N = 8 * 256 * (4 * cus + 1) * 4 * 2 + 3
    colors = P.cyclic_colors(N, 3)
    dcv = torch.as_tensor(colors, device="cuda").to(tdt)
    w = dcv.element_size()
    assert dcv.data_ptr() % 16 == 0
    grids = M.fused_grids((0, 0, N), (8, 8, w), cus)
    assert grids.g[2] == grids.share[2] == 4 * cus + 1 < (N + 2047) // 2048
    cls = M.pair_classes(N, w, 0, 256 * grids.g[2])
    path = M.QUADS if w == 4 else M.VEC
    assert np.any(cls == (path | M.UNROLLED))
    rest = path if np.any(cls == path) else M.QUAD_TAIL
    assert np.any(cls == rest) and (w == 4 or rest == path)
    plan = _tri_plan(N, colors)
    for rep in range(2):
        _stale_after(ctx, plan, (None, None, dcv), False, ("clean", rep))
    for lab, j in (("unrolled", 2 * M.pick(cls, path | M.UNROLLED) + 1), (M.class_name(rest), 2 * M.pick(cls, rest, "first")), ("last element", N - 1)):
        plan = _tri_plan(N, colors)
        dcv[j] += 1
        _stale_after(ctx, plan, (None, None, dcv), True, (lab, j))
        dcv[j] -= 1


def test_deferred_length_mismatch_is_refused_by_the_call(ctx):
    # a resized array cannot be the plan's: refused on the host, before any launch -- FD_ERR_STALE from the call itself, the plan stale,
    # nothing in the context's word
    N = 3001
    colors = P.cyclic_colors(N, 3)
    plan = _tri_plan(N, colors)
    dcv = _dev(colors.astype(np.int32))
    with pytest.raises(fd.lib.FdError) as e:
        plan.matches(colorvec=dcv[:-1], deferred=True)
    assert e.value.code == FD_ERR_STALE and plan.stale()
    ctx.synchronize()
