"""Child process of tests/test_gpu_cscblock.py (not a test file): the block-Jacobi solve on every row of the reaction-diffusion table and
on the block-tridiagonal pattern with 32 x 32 blocks, under FDJAC_CSC_BATCH in {1, 8} x FDJAC_CSC_WINDOW in {0, 1} -- y, the iteration
count, the residual norm and the flags BIT FOR BIT against tests/csc_block_model.py.  The parent starts it with FDJAC_TEST_SWITCHES=1
(the library reads its switches only then); it prints one line per case and "all ok" at the end, and exits non-zero on a mismatch."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import finitediff_jl_amd as fd            # noqa: E402
import csc_solve_model as M               # noqa: E402
import csc_block_model as BM              # noqa: E402
import test_cscblock_model_cpu as H       # noqa: E402


def c5_case():
    """Block-tridiagonal, 40 blocks of 32 x 32 (rows of 96 entries: the long-row product), strong diagonal blocks, weak coupling."""
    colptr, rowval, N = BM.block_tridiag_pattern(40, 32)
    rng = np.random.default_rng(12)
    cols = np.repeat(np.arange(N), np.diff(colptr))
    nz = rng.uniform(-1, 1, rowval.size) * np.where(rowval // 32 == cols // 32, 1.0, 0.05)
    return colptr, rowval, nz, N, rng.standard_normal(N)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def main():
    assert os.environ.get("FDJAC_TEST_SWITCHES") == "1"
    cases = [("table %r" % (c,), c[0], H.family_case(*c)) for c in H.TABLE_SYM + H.TABLE_SKEW] + [("c5 32", 32, c5_case())]
    failures = 0
    for name, bs, (colptr, rowval, nz, N, b) in cases:
        rl = M.RowLists(colptr, rowval, N)
        want, wst = BM.solve(rl, 1.0, -H.GAMMA, nz, b, H.RTOL, H.MAXIT, precond=("block", bs))
        assert wst["flags"] == 0, (name, wst)
        if bs == 32:
            assert rl.nlong > 0
        for batch in ("1", "8"):
            for window in ("0", "1"):
                os.environ["FDJAC_CSC_BATCH"], os.environ["FDJAC_CSC_WINDOW"] = batch, window
                s = fd.CscSolver((colptr, rowval, N), idx_base=0)
                s.set_options(H.RTOL, H.MAXIT)
                s.set_preconditioner("block_jacobi", bs)
                y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
                s.solve(torch.as_tensor(nz, device="cuda"), torch.as_tensor(b, device="cuda"), y, 1.0, -H.GAMMA)
                st = s.status()
                ok = st == wst and np.array_equal(bits(y.cpu().numpy()), bits(want))
                print("%s batch %s window %s: %s iterations %d (model %d) resid %.3e (model %.3e)"
                      % (name, batch, window, "ok" if ok else "MISMATCH", st["iterations"], wst["iterations"], st["resid"], wst["resid"]), flush=True)
                failures += 0 if ok else 1
    if failures:
        print("%d mismatches" % failures)
        return 1
    print("all ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
