"""The cases of tests/test_gpu_jfnk_pc.py and tests/test_jfnk_pc_model_cpu.py: the systems of tests/jfnk_cases.py (x, b as there, alpha = 1,
beta = -GAMMA) solved by the matrix-free consumer with a LAGGED factorisation of the stored Jacobian as its right preconditioner.  Pure
numpy.  Test infrastructure only.

  the lag     the factorisation is of  I - GAMMA0 J(x0)  with x0 = x + 0.05 u (u uniform in [0, 1), a stream of its own) and
              GAMMA0 = 0.25 != GAMMA = 0.3: neither the point nor the shift is the solve's.
  stored J    the family's full pattern (csc_solve_model.tridiag_pattern / lap5_pattern) with the values of jfnk_model.jacobian_dense
              at x0.  jacobian_nz() below states those values entry by entry, so that the sizes above kSmallN need no dense N x N
              array; tests/test_jfnk_pc_model_cpu.py checks it against jacobian_dense on the small sizes.
  kind        ("jacobi",) | ("block", bs) | ("ilu", bs): what is selected on the lent fd_csc_solver when it factors."""
import functools

import numpy as np

import csc_solve_model as M
import jfnk_cases as JK
import jfnk_pc_model as PM

GAMMA = JK.GAMMA
GAMMA0 = 0.25
LAG = 0.05
KINDS = (("jacobi",), ("block", 2), ("block", 5), ("block", 32), ("ilu", 2), ("ilu", 64), ("ilu", 1024))
EDGE_SIZES = (1, 2, 63, 65, 1023, 1025, 2049)
SWITCH_SIZES = (16383, 16384, 16385, 16386)
SMALL_OFF_SIZES = (1, 2, 3, 31, 257, 1025)
RESTARTS = (1, 2, 5, 30)
LAP5_GRIDS = ((4, 5), (7, 9), (130, 131))


def pattern(family, prm):
    return M.tridiag_pattern(prm[0]) if family.startswith("tridiag") else M.lap5_pattern(*prm)


def jacobian_nz(family, prm, x, colptr, rowval):
    """The values of jfnk_model.jacobian_dense(family, prm, x) at the stored positions, in storage order."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    c = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
    r = np.asarray(rowval, dtype=np.int64)
    nl = family.endswith("_nl")
    if family.startswith("tridiag"):
        xp = np.concatenate([x[1:], [0.0]])
        v = np.where(r == c, -2.0, 1.0)
        if nl:
            v = np.where(r == c, v + 2.0 * x[r] * xp[r], v)
            v = np.where(c == r + 1, v + x[r] ** 2, v)
        return v
    nx = prm[0]
    east = (r % nx) + 1 < nx                                   # row k has an eastern neighbour k + 1
    e = np.where(east, x[np.minimum(r + 1, N - 1)], 0.0)
    v = np.where(r == c, -4.0, 1.0)
    if nl:
        v = np.where(r == c, v + 2.0 * x[r] * e, v)
        v = np.where((c == r + 1) & east, v + x[r] ** 2, v)
    return v


@functools.lru_cache(maxsize=None)
def stored(family, prm):
    """(colptr, rowval, RowLists, x0, nz0): the pattern and what the CSC plan stored at x0."""
    _f, x, _b, _d = JK.system(family, prm)
    colptr, rowval, N = pattern(family, prm)
    u = np.random.default_rng(77 + 13 * N + len(family)).random(N)
    x0 = x + LAG * u
    return colptr, rowval, M.RowLists(colptr, rowval, N), x0, jacobian_nz(family, prm, x0, colptr, rowval)


def _case(family, prm, kind, fdtype="forward", fin=False, route="plain", xoff=0, restart=30, maxit=8, rtol=JK.RTOL, small_off=False):
    prm = tuple(prm)
    if route != "plain" and not JK.has_lazy(family, prm):
        route = "plain"
    c = dict(family=family, prm=prm, kind=tuple(kind), fdtype=fdtype, fin=fin, route=route, xoff=xoff, restart=restart, maxit=maxit, rtol=rtol,
             small_off=small_off)
    c["id"] = "-".join([family, "x".join(map(str, prm)), "".join(map(str, kind)), fdtype, route, "m%d" % restart, "it%d" % maxit] +
                       [t for t, on in (("fin", fin), ("xoff", xoff), ("small0", small_off)) if on])
    return c


def _build():
    out = []
    fd2, routes, fams = ("forward", "central"), ("plain", "lazy", "quot"), ("tridiag", "tridiag_nl")
    # the tile and block edges: every size on both tridiagonal families, the kinds, routes, arms and restarts rotating
    for f, fam in enumerate(fams):
        for i, n in enumerate(EDGE_SIZES):
            k = i + 3 * f
            out.append(_case(fam, (n,), KINDS[k % 7], fd2[(i + f) % 2], fin=k % 3 == 0, route=routes[(i + f) % 3], xoff=(i // 2) % 2,
                             restart=RESTARTS[k % 4], maxit=8))
    # the kSmallN switch: block Jacobi on every route, 32 and 5, x on a pair and off it (odd N on the fused kernel's paired and scalar
    # variants and its tail)
    for i, n in enumerate(SWITCH_SIZES):
        for k, r in enumerate(routes):
            out.append(_case(fams[(i + k) % 2], (n,), ("block", (32, 5)[(i + k) % 2]), fd2[(i + k) % 2], fin=(i + k) % 3 == 1, route=r,
                             xoff=(i + k) % 3 == 2, restart=(5, 30, 2)[k], maxit=6))
    for bs in (32, 5):
        for xoff in (0, 1):
            out.append(_case("tridiag_nl", (16385,), ("block", bs), "forward", route="quot", xoff=xoff, restart=5, maxit=5))
    # the fused kernel at small sizes (FDJAC_SMALL=0): one partial, a block that straddles a trip, a last block of one row
    for i, n in enumerate(SMALL_OFF_SIZES):
        out.append(_case(fams[i % 2], (n,), ("block", (2, 5, 32)[i % 3]), fd2[i % 2], route=routes[i % 3], xoff=i % 2, restart=5, maxit=8, small_off=True))
    for n in (257, 1025):
        for k, bs in enumerate((5, 32, 2)):
            out.append(_case(fams[k % 2], (n,), ("block", bs), fd2[(k + 1) % 2], route=routes[(k + 1) % 3], xoff=(k + 1) % 2, restart=2, maxit=6,
                             small_off=True))
    # the 5-point families: ILU 1024 and block 32 on every grid, the diagonal on the smallest
    for g, grid in enumerate(LAP5_GRIDS):
        for k, fam in enumerate(("lap5", "lap5_nl")):
            for q, kind in enumerate((("ilu", 1024), ("block", 32))):
                out.append(_case(fam, grid, kind, fd2[(g + k + q) % 2], fin=(g + q) % 2 == 0, route=routes[(g + k + q) % 3], xoff=(g + k) % 2,
                                 restart=(5, 30)[q], maxit=6))
    out += [_case("lap5", (4, 5), ("jacobi",), "central", route="quot", restart=5, maxit=8),
            _case("lap5_nl", (4, 5), ("jacobi",), "forward", fin=True, route="lazy", xoff=1, restart=2, maxit=8),
            _case("lap5", (7, 9), ("ilu", 64), "forward", restart=30, maxit=8),
            _case("lap5", (130, 131), ("block", 32), "forward", fin=True, route="quot", restart=5, maxit=5),
            _case("lap5_nl", (130, 131), ("ilu", 1024), "central", route="lazy", xoff=1, restart=5, maxit=5)]
    seen, uniq = set(), []
    for c in out:
        if c["id"] not in seen:
            seen.add(c["id"])
            uniq.append(c)
    return uniq


CASES = _build()


def model(case, num_cus=256, keep=True, fault=None, trace=None, maxit=None, rtol=None, lagged=None, x=None, kind=None):
    """The model's (y, status) of a case; lagged replaces (1, -GAMMA0, nz0), x the solve's point, kind the case's."""
    f, x1, b, _d = JK.system(case["family"], case["prm"])
    x = x1 if x is None else x
    colptr, rowval, rl, _x0, nz0 = stored(case["family"], case["prm"])
    with np.errstate(all="ignore"):
        fin = f(x) if case["fin"] and case["fdtype"] == "forward" else None
    nz_now = jacobian_nz(case["family"], case["prm"], x, colptr, rowval) if fault == "factor_at_x1" else None
    return PM.solve(f, x, b, 1.0, -GAMMA, rl, (1.0, -GAMMA0, nz0) if lagged is None else lagged, case["kind"] if kind is None else kind,
                    case["fdtype"], case["rtol"] if rtol is None else rtol, case["maxit"] if maxit is None else maxit, keep, case["restart"],
                    num_cus, f_in=fin, x_aligned=not case["xoff"], small_off=case["small_off"], fault=fault, trace=trace, nz_now=nz_now)
