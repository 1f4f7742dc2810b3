"""The cases of tests/test_gpu_jfnk.py and tests/test_jfnk_model_cpu.py: systems (alpha I + beta J(x)) y = b on the built-in square families
that tests/jvp_cases.py models, the table of routes, and the model's answer per case.  Pure numpy.  Test infrastructure only.

  system      x in [-0.25, 0.75) (jvp_cases' generic operands), b in [-1, 1], alpha = 1, beta = -gamma: I - gamma J.  J of the linear
              families has its spectrum in [-4, 0] (tridiagonal) / [-8, 0] (5-point), so I - gamma J is positive definite with a condition
              number of at most 1 + 8 gamma; the nonlinear terms x_i^2 x_i+1 move the entries by less than 1.2.  GAMMA = 0.3.
  diagonal    d = 1 + gamma (2 | 4) (1 + 0.1 u), u in [0, 1): close to the diagonal of I - gamma J, never zero.
  route       plain (no lazy launcher), lazy (values), quot (the launcher writes the quotient); forward / central; f_in given or not;
              the diagonal set or not; x, b and d offset by one element (misaligned to a pair) or not.  EVERY family runs every value of
              each of these (f_in counted in the forward arm only, where it is read): tests/test_gpu_jfnk.py::test_the_cases_cover."""
import functools

import numpy as np

import exact_model as X
import jfnk_model as JM
import jvp_cases as JC
import jvp_model as J

GAMMA = 0.3           # (not a power of two: beta q is rounded)
RTOL = 1e-6
TILE_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
SWITCH_SIZES = (16383, 16384, 16385, 16386)
RESTARTS = (1, 2, 5, 30, 64)
LAP5_GRIDS = ((4, 5), (7, 9), (130, 131), (131, 131))          # even nx: a lazy launcher; odd nx: none; the last two above kSmallN


def size_of(family, prm):
    return prm[0] if family.startswith("tridiag") else prm[0] * prm[1]


def has_lazy(family, prm):
    return family.startswith("tridiag") or prm[0] % 2 == 0


@functools.lru_cache(maxsize=None)
def system(family, prm):
    """(f, x, b, d) of the family at its size."""
    N = size_of(family, prm)
    rng = np.random.default_rng(1000003 * len(family) + 31 * N + prm[0])
    x = rng.random(N) - 0.25
    b = rng.uniform(-1.0, 1.0, N)
    d = 1.0 + GAMMA * (2.0 if family.startswith("tridiag") else 4.0) * (1.0 + 0.1 * rng.random(N))
    return X.fixture(family, *prm), x, b, d


def _case(family, prm, fdtype="forward", fin=False, route="plain", diag=False, xoff=0, boff=0, doff=0, restart=30, maxit=12, rtol=RTOL,
          small_off=False):
    prm = tuple(prm)
    if route != "plain" and not has_lazy(family, prm):
        route = "plain"
    c = dict(family=family, prm=prm, fdtype=fdtype, fin=fin, route=route, diag=diag, xoff=xoff, boff=boff, doff=doff, restart=restart,
             maxit=maxit, rtol=rtol, small_off=small_off)
    c["id"] = "-".join([family, "x".join(map(str, prm)), fdtype, route, "m%d" % restart, "it%d" % maxit] +
                       [t for t, on in (("fin", fin), ("diag", diag), ("xoff", xoff), ("boff", boff), ("doff", doff), ("small0", small_off)) if on])
    return c


def _build():
    out = []
    fd2, routes, fams = ("forward", "central"), ("plain", "lazy", "quot"), ("tridiag", "tridiag_nl")
    # the tile edges of kCsVecTile: every size once, the routes, restarts and offsets rotating; enough steps for every restart to restart
    for i, n in enumerate(TILE_SIZES):
        out.append(_case(fams[i % 2], (n,), fd2[i % 2], fin=i % 3 == 0, route=routes[i % 3], diag=i % 2 == 1, xoff=(i // 2) % 2, boff=(i // 3) % 2,
                         doff=(i // 4) % 2, restart=RESTARTS[i % 5], maxit=12))
    # the kSmallN switch, with an odd N on the large route: every route there, the diagonal set and unset, aligned and not
    for i, n in enumerate(SWITCH_SIZES):
        for k, r in enumerate(routes):
            out.append(_case(fams[(i + k) % 2], (n,), fd2[(i + k) % 2], fin=(i + k) % 3 == 1, route=r, diag=(i + k) % 2 == 0, xoff=(i + k) % 3 == 2,
                             doff=k == 0 and i % 2 == 1, restart=(5, 30, 2)[k], maxit=7))
    for n in (16385, 16386):          # forward and central, f_in given and not, on each route above kSmallN, both with the diagonal
        for fdt in fd2:
            for fin in (False, True):
                for r in routes:
                    out.append(_case("tridiag_nl", (n,), fdt, fin=fin, route=r, diag=True, restart=5, maxit=6))
    # the opening kernel's scalar variant by each of its causes on an odd N: a misaligned d, a misaligned x
    out.append(_case("tridiag", (16385,), "forward", route="lazy", diag=True, doff=1, restart=5, maxit=6))
    out.append(_case("tridiag_nl", (16385,), "central", route="plain", diag=True, xoff=1, restart=5, maxit=6))
    # the large kernels at small sizes (FDJAC_SMALL=0): the opening kernel's tail, one partial
    for i, n in enumerate((1, 2, 3, 257, 1025)):
        out.append(_case(fams[i % 2], (n,), fd2[i % 2], route=routes[i % 3], diag=True, xoff=i % 2, doff=(i // 2) % 2, restart=5, maxit=8, small_off=True))
    # the 5-point families
    for g, grid in enumerate(LAP5_GRIDS):
        for k, fam in enumerate(("lap5", "lap5_nl")):
            out.append(_case(fam, grid, fd2[(g + k) % 2], fin=k == 1 and g % 2 == 0, route=routes[(g + k) % 3], diag=(g + k) % 2 == 0, xoff=0,
                             boff=g % 2, restart=(5, 30)[k], maxit=8))
    out.append(_case("lap5_nl", (130, 131), "forward", route="quot", diag=True, xoff=1, restart=5, maxit=6))
    out.append(_case("lap5", (130, 131), "central", route="lazy", diag=False, restart=2, maxit=5))
    # what the rotations above leave out, family by family: the tridiagonal family's central arm; a caller's f_in in the forward arm of
    # the 5-point families (the lazy launcher then writes values: small, above kSmallN on an even nx, and without a launcher); lap5 with x
    # off a pair; each 5-point family on each route
    out += [_case("tridiag", (1025,), "central", route="quot", diag=True, restart=5, maxit=8),
            _case("tridiag", (16385,), "central", route="lazy", diag=True, xoff=1, restart=5, maxit=6),
            _case("tridiag", (16386,), "central", route="plain", restart=2, maxit=5),
            _case("lap5", (4, 5), "forward", fin=True, route="lazy", restart=5, maxit=8),
            _case("lap5", (130, 131), "forward", fin=True, route="quot", diag=True, restart=5, maxit=6),
            _case("lap5", (130, 131), "forward", fin=True, route="lazy", xoff=1, restart=2, maxit=5),
            _case("lap5", (131, 131), "forward", fin=True, route="plain", diag=True, xoff=1, doff=1, restart=5, maxit=6),
            _case("lap5_nl", (4, 5), "forward", fin=True, route="quot", diag=True, restart=5, maxit=8),
            _case("lap5_nl", (130, 131), "forward", fin=True, route="quot", restart=5, maxit=6),
            _case("lap5_nl", (130, 131), "forward", fin=True, route="lazy", diag=True, doff=1, boff=1, restart=2, maxit=5),
            _case("lap5_nl", (130, 131), "central", route="lazy", diag=True, restart=5, maxit=6),
            _case("lap5_nl", (131, 131), "forward", fin=True, route="plain", xoff=1, restart=5, maxit=6),
            _case("lap5", (130, 131), "forward", route="plain", diag=True, boff=1, restart=5, maxit=6),
            _case("tridiag", (2049,), "forward", fin=True, route="plain", boff=1, restart=5, maxit=8),
            _case("tridiag_nl", (2049,), "forward", route="lazy", boff=1, restart=5, maxit=8)]
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _build()

# convergence: solved to RTOL; the CPU suite checks that the model ends with flags 0, the GPU suite the true residual
CONVERGENCE = [_case("tridiag", (255,), "forward", route="quot", restart=30, maxit=200),
               _case("tridiag_nl", (1025,), "central", route="lazy", diag=True, restart=5, maxit=200),          # at least three cycles
               _case("tridiag_nl", (257,), "forward", fin=True, restart=64, maxit=200),
               _case("lap5", (9, 7), "forward", diag=True, restart=5, maxit=200),
               _case("lap5_nl", (16, 15), "central", route="quot", restart=30, maxit=200),
               _case("lap5_nl", (4, 5), "forward", route="lazy", diag=True, xoff=1, restart=2, maxit=200)]


def model(case, num_cus=JC.SEARCH_CUS, keep=True, fault=None, trace=None, maxit=None, rtol=None, restart=None, b=None, d=None, x=None):
    """The model's (y, status) of a case; b / d / x replace the system's."""
    f, x0, b0, d0 = system(case["family"], case["prm"])
    x = x0 if x is None else x
    with np.errstate(all="ignore"):
        fin = f(x) if case["fin"] and case["fdtype"] == "forward" else None
    dd = (d0 if d is None else d) if case["diag"] else None
    return JM.solve(f, x, b0 if b is None else b, 1.0, -GAMMA, case["fdtype"], dd, case["rtol"] if rtol is None else rtol,
                    case["maxit"] if maxit is None else maxit, keep, case["restart"] if restart is None else restart, num_cus,
                    f_in=fin, x_aligned=not case["xoff"], small_off=case["small_off"], fault=fault, trace=trace)
