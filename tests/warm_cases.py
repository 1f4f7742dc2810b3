"""The inputs of tests/test_gpu_warm_start.py, shared with tests/test_warm_model_cpu.py (which shows that these inputs tell the deliberately
wrong model variants from the right one, and that the implicit-step sequence saves iterations in the model).  Pure numpy.  Test
infrastructure only.

  sparse systems   values, b and y0 in [-1, 1] (streams of their own), A = I - gamma J with gamma * max ||row of J||_1 = 0.9, as the
                   existing GPU tests of the sparse consumer scale theirs.  y0 is a GUESS, not a good one: the start has to be right for
                   any y0.  Sizes: 1, 2, 3; lap5 12 x 11 (N = 132: bs = 8 and bs = 50 leave a short last block); 1023, 1024, 1025 (one
                   below, at and above kCsVecTile) and 2049 on the tridiagonal pattern; odd_pattern with a dense row of 33 entries (one
                   past kCsLong) and of 300 (more than one trip of the workgroup's strided sum).
  the sequence     (I - gamma J) u+ = u on lap5 12 x 11, 4 steps, cold and from y0 = b (below: which J and which first state, and why)."""
import functools

import numpy as np

import csc_solve_model as M
import jfnk_cases as JK
import jfnk_pc_cases as PC

RESTART = 5           # GMRES: restarts happen behind the warm first cycle
MAXIT = 40
SIZES = ("1", "2", "3", "lap5", "1023", "1024", "1025", "2049", "odd33", "odd300")
METHODS = ("bicgstab", "gmres")
PRECONDS = (("jacobi",), ("block", 8), ("ilu", 50))


@functools.lru_cache(maxsize=None)
def system(name):
    """(colptr, rowval, N, nz, b, y0, gamma, RowLists)."""
    if name == "lap5":
        colptr, rowval, N = M.lap5_pattern(12, 11)
    elif name == "odd33":
        colptr, rowval, N = M.odd_pattern(300, 77, 33, 1)
    elif name == "odd300":
        colptr, rowval, N = M.odd_pattern(1100, 502, 300, 2)
    else:
        colptr, rowval, N = M.tridiag_pattern(int(name))
    rng = np.random.default_rng(4000 + N)
    nz = rng.uniform(-1.0, 1.0, rowval.size)
    b = rng.uniform(-1.0, 1.0, N)
    y0 = rng.uniform(-1.0, 1.0, N)
    rows = np.zeros(N)
    np.add.at(rows, rowval, np.abs(nz))
    return colptr, rowval, N, nz, b, y0, float(0.9 / rows.max()), M.RowLists(colptr, rowval, N)


def rtol_of(dtype):
    return 1e-10 if np.dtype(dtype) == np.float64 else 1e-6


# every size x method x preconditioner x element type
SPARSE_CASES = [(n, m, pc, dt) for n in SIZES for m in METHODS for pc in PRECONDS for dt in (np.float64, np.float32)]

# ---- the implicit-step sequence ----------------------------------------------------------------------------------------------------------
# (I - gamma J) u+ = u, four steps.  With ONE diffusion coefficient y0 = b saves nothing in the model at any gamma from 0.25 to 16: the
# stopping rule is relative to ||b||, r0 = -gamma J b is no smaller than b where gamma ||J|| > 1, and where it is smaller the cold solve
# needs fewer than 10 iterations.  A guess pays where the stiffness and the state live apart: J = diag(c) * (5-point Laplacian) with c = 1
# in the 6 x 6 corner of the grid and 1e-4 elsewhere, gamma = 100 (the corner is what makes the cold solve long), and a first state that is
# zero on the corner and its rim, so that J u is small.  tests/test_warm_model_cpu.py checks the counts this gives in the model.
SEQ_GRID, SEQ_GAMMA, SEQ_STEPS, SEQ_RTOL, SEQ_CORNER, SEQ_C = (12, 11), 100.0, 4, 1e-10, 6, (1.0, 1e-4)


@functools.lru_cache(maxsize=None)
def sequence():
    """(colptr, rowval, N, nz, u0, RowLists) of the sequence above."""
    nx = SEQ_GRID[0]
    colptr, rowval, N = M.lap5_pattern(*SEQ_GRID)
    cols = np.repeat(np.arange(N), np.diff(colptr))
    k = np.arange(N)
    i, j = k % nx, k // nx
    c = np.where((i < SEQ_CORNER) & (j < SEQ_CORNER), SEQ_C[0], SEQ_C[1])
    nz = np.where(rowval == cols, -4.0, 1.0) * c[rowval]
    u0 = np.where((i < SEQ_CORNER + 1) & (j < SEQ_CORNER + 1), 0.0, np.random.default_rng(12).uniform(-1.0, 1.0, N))
    return colptr, rowval, N, nz, u0, M.RowLists(colptr, rowval, N)


# ---- the matrix-free consumer: the families of tests/jfnk_cases.py at their smallest sizes ------------------------------------------------
def _jf(family, prm, fdtype, pc, restart=RESTART, maxit=12):
    kind = None if pc in (None, "diag") else pc
    c = dict(family=family, prm=tuple(prm), fdtype=fdtype, pc=pc, kind=kind, restart=restart, maxit=maxit, rtol=JK.RTOL)
    c["id"] = "-".join([family, "x".join(map(str, prm)), fdtype, "none" if pc is None else (pc if pc == "diag" else "".join(map(str, pc)))])
    return c


JFNK_CASES = [_jf(fam, prm, fdt, pc)
              for fam, prm in (("tridiag", (1,)), ("tridiag_nl", (2,)), ("lap5", (4, 5)), ("lap5_nl", (4, 5)), ("tridiag_nl", (1025,)))
              for fdt in ("forward", "central") for pc in (None, "diag", ("block", 5))]


@functools.lru_cache(maxsize=None)
def jfnk_system(family, prm):
    """(f, x, b, d, y0): tests/jfnk_cases.py's system and a guess in [-1, 1]."""
    f, x, b, d = JK.system(family, prm)
    y0 = np.random.default_rng(515 + x.size).uniform(-1.0, 1.0, x.size)
    return f, x, b, d, y0


def client_sequence():
    """The sequence as examples/csc_warm_client.c builds it: the same J, and a first state from integer arithmetic (exact in C and here)."""
    colptr, rowval, N, nz, _u0, rl = sequence()
    k = np.arange(N)
    i, j = k % SEQ_GRID[0], k // SEQ_GRID[0]
    u0 = np.where((i < SEQ_CORNER + 1) & (j < SEQ_CORNER + 1), 0.0, ((k * 37 + 11) % 101) / 50.0 - 1.0)
    return colptr, rowval, N, nz, u0, rl


def jfnk_lent(case):
    """What warm_model.jfnk_solve takes as `lent` for a case with a lent factorisation: tests/jfnk_pc_cases.py's lagged stored J."""
    _colptr, _rowval, rl, _x0, nz0 = PC.stored(case["family"], case["prm"])
    return rl, (1.0, -PC.GAMMA0, nz0), case["kind"]
