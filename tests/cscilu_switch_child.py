"""Child process of tests/test_gpu_cscilu.py (not a test file): the block-ILU(0) solve on the 5-point and the ragged case under
FDJAC_CSC_BATCH in {1, 8} x FDJAC_CSC_WINDOW in {0, 1} -- y, the iteration count, the residual norm and the flags BIT FOR BIT against
tests/csc_ilu_model.py.  The parent starts it with FDJAC_TEST_SWITCHES=1 (the library reads its switches only then); it prints one line
per case and "all ok" at the end, and exits non-zero on a mismatch."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import finitediff_jl_amd as fd            # noqa: E402
import csc_solve_model as M               # noqa: E402
import csc_ilu_model as IM                # noqa: E402
import test_cscilu_model_cpu as H         # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def main():
    assert os.environ.get("FDJAC_TEST_SWITCHES") == "1"
    colptr, rowval, N, nz, b, gamma = H.grid_case("convdiff_g50", 12, 9)
    cases = [("5-point 12 x 9", (colptr, rowval, N, nz, b, gamma), (36, 64)), ("ragged 300", H.ragged_case(), (64, 256))]
    failures = 0
    for name, (colptr, rowval, N, nz, b, gamma), sizes in cases:
        rl = M.RowLists(colptr, rowval, N)
        for bs in sizes:
            want, wst = IM.solve(rl, 1.0, -gamma, nz, b, H.RTOL, H.MAXIT, bs=bs)
            assert wst["flags"] == 0 and wst["iterations"] >= 2, (name, wst)
            for batch in ("1", "8"):
                for window in ("0", "1"):
                    os.environ["FDJAC_CSC_BATCH"], os.environ["FDJAC_CSC_WINDOW"] = batch, window
                    s = fd.CscSolver((colptr, rowval, N), idx_base=0)
                    s.set_options(H.RTOL, H.MAXIT)
                    s.set_block_ilu(bs)
                    y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
                    s.solve(torch.as_tensor(nz, device="cuda"), torch.as_tensor(b, device="cuda"), y, 1.0, -gamma)
                    st = s.status()
                    ok = st == wst and np.array_equal(bits(y.cpu().numpy()), bits(want))
                    print("%s bs %d batch %s window %s: %s iterations %d (model %d) resid %.3e (model %.3e)"
                          % (name, bs, batch, window, "ok" if ok else "MISMATCH", st["iterations"], wst["iterations"], st["resid"], wst["resid"]), flush=True)
                    failures += 0 if ok else 1
    if failures:
        print("%d mismatches" % failures)
        return 1
    print("all ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
