"""The cases of tests/test_gpu_jftr.py, tests/jftr_switch_child.py and tests/test_jftr_model_cpu.py: trust-region steps on the built-in
square families that tests/jvp_cases.py models (jfnk_cases.system hands out f, x, a right-hand side and a positive diagonal), the table of
routes and exits, and the model's answer per case.  Pure numpy.  Test infrastructure only.

  the model   B = lam I + beta J(x).  J of the linear families (tridiag, lap5) is constant and symmetric with its spectrum in [-4, 0] /
              [-8, 0]: with beta = -1, lam = 1/2, B is positive definite (spectrum in [0.5, 4.5] / [0.5, 8.5]); with beta = +1, lam = 0 it
              is negative definite.  The nonlinear families' J is not symmetric: their steps are compared with the model only.
  g, m        g = the system's right-hand side in [-1, 1]; m = its diagonal (1 + 0.3 (2 | 4) (1 + 0.1 u) > 0), offset by one element or not.
  radius      "inf", an absolute number, or ("rel", f): f times ||y*||_W of the model's own interior step (radius "inf") of that case.
  route       plain / lazy (values) / quot; forward with and without f_in, central; m set and unset; x and m on and off a pair.  EVERY
              family runs every value of each of these: tests/test_gpu_jftr.py::test_the_cases_cover."""
import numpy as np

import jfnk_cases as JK
import jftr_model as TR
import jvp_cases as JC

RTOL, MAXIT = 1e-6, 200
INF = float("inf")
TILE_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
SWITCH_SIZES = JK.SWITCH_SIZES
LAP5_GRIDS = JK.LAP5_GRIDS
FAMILIES = ("tridiag", "tridiag_nl", "lap5", "lap5_nl")
# (lam, beta, radius) by the exit they lead to on the linear families
INTERIOR = ((0.5, -1.0, "inf"), (0.5, -1.0, ("rel", 2.0)))
BOUNDARY = ((0.5, -1.0, ("rel", 0.5)), (0.5, -1.0, ("rel", 0.1)), (0.5, -1.0, ("rel", 1e-3)))
NEGATIVE = ((0.0, 1.0, 100.0),)
UNBOUNDED = ((0.0, 1.0, "inf"),)
WANT_EXIT = dict([(e, 0) for e in INTERIOR] + [(e, 1) for e in BOUNDARY] + [(e, 2) for e in NEGATIVE] + [(e, 3) for e in UNBOUNDED])
ROTATION = INTERIOR + BOUNDARY + NEGATIVE + UNBOUNDED

size_of, has_lazy, system = JK.size_of, JK.has_lazy, JK.system


def _case(family, prm, fdtype="forward", fin=False, route="plain", diag=False, xoff=0, moff=0, model=INTERIOR[0], maxit=MAXIT, rtol=RTOL,
          small_off=False, fuse=True):
    prm = tuple(prm)
    if route != "plain" and not has_lazy(family, prm):
        route = "plain"
    lam, beta, radius = model
    c = dict(family=family, prm=prm, fdtype=fdtype, fin=fin, route=route, diag=diag, xoff=xoff, moff=moff, lam=lam, beta=beta, radius=radius,
             maxit=maxit, rtol=rtol, small_off=small_off, fuse=fuse)
    rad = radius if isinstance(radius, str) else ("%gy" % radius[1] if isinstance(radius, tuple) else "%g" % radius)
    c["id"] = "-".join([family, "x".join(map(str, prm)), fdtype, route, "l%g" % lam, "b%g" % beta, "r" + rad, "it%d" % maxit] +
                       [t for t, on in (("fin", fin), ("diag", diag), ("xoff", xoff), ("moff", moff), ("small0", small_off), ("nofuse", not fuse)) if on])
    return c


def _build():
    out = []
    fd2, routes, fams = ("forward", "central"), ("plain", "lazy", "quot"), ("tridiag", "tridiag_nl")
    # the tile edges of kCsVecTile: every size once; the routes, the exits and the offsets rotating
    for i, n in enumerate(TILE_SIZES):
        out.append(_case(fams[i % 2], (n,), fd2[i % 2], fin=i % 3 == 0, route=routes[i % 3], diag=i % 2 == 1, xoff=(i // 2) % 2, moff=(i // 4) % 2,
                         model=ROTATION[i % len(ROTATION)]))
    # the kSmallN switch, with an odd N on the large route: every route there, m set and unset, x and m on and off a pair
    for i, n in enumerate(SWITCH_SIZES):
        for k, r in enumerate(routes):
            out.append(_case(fams[(i + k) % 2], (n,), fd2[(i + k) % 2], fin=(i + k) % 3 == 1, route=r, diag=(i + k) % 2 == 0, xoff=(i + k) % 3 == 2,
                             moff=k == 0 and i % 2 == 1, model=ROTATION[(3 * i + k) % len(ROTATION)], maxit=12))
    for n in (16385, 16386):          # forward and central, f_in given and not, on each route above kSmallN
        for fdt in fd2:
            for fin in (False, True):
                for r in routes:
                    out.append(_case("tridiag_nl", (n,), fdt, fin=fin, route=r, diag=r != "lazy", model=INTERIOR[0], maxit=6))
    # k_jt_p's scalar variant (x off a pair) on an odd and an even N; m off a pair above kSmallN
    out.append(_case("tridiag", (16385,), "forward", route="lazy", diag=True, xoff=1, model=BOUNDARY[0], maxit=12))
    out.append(_case("tridiag_nl", (16386,), "central", route="plain", diag=True, xoff=1, moff=1, model=INTERIOR[0], maxit=6))
    out.append(_case("tridiag", (16385,), "central", route="quot", diag=True, moff=1, model=INTERIOR[1], maxit=8))
    # the 5-point families
    for gi, grid in enumerate(LAP5_GRIDS):
        for k, fam in enumerate(("lap5", "lap5_nl")):
            out.append(_case(fam, grid, fd2[(gi + k) % 2], fin=k == 1 and gi % 2 == 0, route=routes[(gi + k) % 3], diag=(gi + k) % 2 == 0,
                             moff=gi % 2, model=ROTATION[(2 * gi + k) % 5], maxit=10 if gi >= 2 else MAXIT))
    # what the rotations above leave out, family by family
    out += [_case("tridiag", (1025,), "central", route="quot", diag=True, model=BOUNDARY[1]),
            _case("tridiag", (2049,), "forward", fin=True, route="plain", model=INTERIOR[1]),
            _case("tridiag", (16386,), "central", route="plain", model=NEGATIVE[0], maxit=5),
            _case("tridiag_nl", (2049,), "forward", route="lazy", xoff=1, model=BOUNDARY[2]),
            _case("lap5", (4, 5), "forward", fin=True, route="lazy", xoff=1, model=INTERIOR[0]),
            _case("lap5", (4, 5), "central", route="quot", diag=True, model=BOUNDARY[0]),
            _case("lap5", (7, 9), "forward", fin=True, route="plain", diag=True, moff=1, model=UNBOUNDED[0]),
            _case("lap5", (130, 131), "forward", fin=True, route="quot", diag=True, model=INTERIOR[0], maxit=8),
            _case("lap5", (130, 131), "forward", route="plain", xoff=1, model=BOUNDARY[1], maxit=8),
            _case("lap5", (131, 131), "central", route="plain", diag=True, xoff=1, moff=1, model=NEGATIVE[0], maxit=5),
            _case("lap5_nl", (4, 5), "forward", fin=True, route="quot", diag=True, xoff=1, model=INTERIOR[0]),
            _case("lap5_nl", (4, 5), "central", route="lazy", model=BOUNDARY[0]),
            _case("lap5_nl", (130, 131), "forward", fin=True, route="lazy", diag=True, moff=1, model=INTERIOR[0], maxit=8),
            _case("lap5_nl", (130, 131), "central", route="quot", model=INTERIOR[0], maxit=8),
            _case("lap5_nl", (130, 131), "forward", route="plain", xoff=1, model=BOUNDARY[0], maxit=8),
            _case("lap5_nl", (131, 131), "forward", fin=True, route="plain", xoff=1, model=INTERIOR[0], maxit=6)]
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _build()

# every exit on a linear family, both norms, small and above kSmallN
EXITS = [_case(fam, prm, fdt, route=route, diag=diag, model=mdl, maxit=MAXIT if size_of(fam, prm) <= 16384 else 40)
         for fam, prm, fdt, route in (("tridiag", (1025,), "forward", "quot"), ("lap5", (130, 131), "central", "lazy"))
         for diag in (False, True) for mdl in ROTATION]

# the large kernels at small sizes (FDJAC_SMALL=0), and the unfused pair above kSmallN (FDJAC_JFTR_FUSE=0): tests/jftr_switch_child.py
SWITCHED = [_case(("tridiag", "tridiag_nl")[i % 2], (n,), ("forward", "central")[i % 2], route=("plain", "lazy", "quot")[i % 3], diag=i % 2 == 0,
                  xoff=i % 2, moff=(i // 2) % 2, model=(INTERIOR[0], BOUNDARY[0], INTERIOR[1], BOUNDARY[1], INTERIOR[0])[i], small_off=True)
            for i, n in enumerate((1, 2, 3, 257, 1025))]
SWITCHED += [_case("tridiag", (1025,), "forward", route="quot", diag=True, model=INTERIOR[0], small_off=True, fuse=False),
             _case("tridiag_nl", (16385,), "central", route="lazy", diag=True, model=INTERIOR[0], maxit=8, fuse=False),
             _case("lap5", (130, 131), "forward", route="quot", xoff=1, model=BOUNDARY[0], maxit=8, fuse=False)]

_models = {}


def operands(case):
    """(f, x, g, m) of a case."""
    return system(case["family"], case["prm"])


def radius_of(case, num_cus=JC.SEARCH_CUS):
    r = case["radius"]
    if r == "inf":
        return INF
    if isinstance(r, tuple):
        inner = dict(case, radius="inf", maxit=MAXIT, id=case["id"] + "*")
        return r[1] * model(inner, num_cus)[2]["step_norm"]
    return float(r)


def model(case, num_cus=JC.SEARCH_CUS, keep=True, maxit=None, rtol=None, x=None, g=None, m=None, radius=None, trace=None, counts=None):
    """The model's (y, r_out, status) of a case; x / g / m / radius replace the case's.  The plain call is computed once and kept."""
    plain = all(v is None for v in (maxit, rtol, x, g, m, radius, trace, counts)) and keep
    key = (case["id"], num_cus)
    if plain and key in _models:
        return _models[key]
    f, x0, g0, m0 = operands(case)
    x = x0 if x is None else x
    with np.errstate(all="ignore"):
        fin = f(x) if case["fin"] and case["fdtype"] == "forward" else None
    mm = (m0 if m is None else m) if case["diag"] else None
    out = TR.step(f, x, g0 if g is None else g, case["lam"], case["beta"], radius_of(case, num_cus) if radius is None else radius, case["fdtype"], mm,
                  case["rtol"] if rtol is None else rtol, case["maxit"] if maxit is None else maxit, keep, num_cus, f_in=fin,
                  x_aligned=not case["xoff"], small_off=case["small_off"], fuse=case["fuse"], trace=trace, counts=counts)
    if plain:
        _models[key] = out
    return out
