"""Child process of tests/test_gpu_csclsq.py (not a test file): the least-squares solve on both rect_band cases for the four (mu, W) pairs
under FDJAC_CSC_BATCH in {1, 8} -- y, r_out, the iteration count, both norms and the flags BIT FOR BIT against tests/csc_lsq_model.py.
The parent starts it with FDJAC_TEST_SWITCHES=1 (the library reads its switches only then); it prints one line per case and "all ok" at
the end, and exits non-zero on a mismatch."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import finitediff_jl_amd as fd                # noqa: E402
import csc_lsq_model as LM                    # noqa: E402
import test_csclsq_model_cpu as H             # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def main():
    assert os.environ.get("FDJAC_TEST_SWITCHES") == "1"
    failures = 0
    for name in ("big", "padded"):
        colptr, rowval, nz, M, N, b, rl = H.band_case(name)
        nzd, bd = torch.as_tensor(nz, device="cuda"), torch.as_tensor(b, device="cuda")
        for mu, kind in LM.MU_W:
            want_y, want_r, wst = H.model_solution(name, mu, kind)
            assert wst["flags"] == 0, (name, mu, kind, wst)
            for batch in ("1", "8"):
                os.environ["FDJAC_CSC_BATCH"] = batch
                s = fd.CscLeastSquares((colptr, rowval, M, N), idx_base=0)
                s.set_options(H.RTOL, H.MAXIT)
                y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
                r = torch.full((M,), 7.0, dtype=torch.float64, device="cuda")
                s.solve(nzd, bd, y, mu, kind, r_out=r)
                st = s.status()
                ok = st == wst and np.array_equal(bits(y.cpu().numpy()), bits(want_y)) and np.array_equal(bits(r.cpu().numpy()), bits(want_r))
                print("%s mu %g kind %d batch %s: %s iterations %d (model %d) grad %.3e (model %.3e)"
                      % (name, mu, kind, batch, "ok" if ok else "MISMATCH", st["iterations"], wst["iterations"], st["grad"], wst["grad"]), flush=True)
                failures += 0 if ok else 1
    if failures:
        print("%d mismatches" % failures)
        return 1
    print("all ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
