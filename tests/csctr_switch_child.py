"""Child process of tests/test_gpu_csctr.py (not a test file): every trust-region step case of tests/test_csctr_model_cpu.py under
FDJAC_CSC_BATCH in {1, 8} -- y, r_out, the exit kind, the flags, the iteration count and the four status scalars BIT FOR BIT against
tests/csc_tr_model.py.  The parent starts it with FDJAC_TEST_SWITCHES=1 (the library reads its switches only then); it prints one line per
case and "all ok" at the end, and exits non-zero on a mismatch."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import finitediff_jl_amd as fd                # noqa: E402
import csc_tr_model as TM                     # noqa: E402
import test_csctr_model_cpu as H              # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def main():
    assert os.environ.get("FDJAC_TEST_SWITCHES") == "1"
    failures = 0
    for name, lam, kind, radius in H.ALL_STEPS:
        colptr, rowval, nz, N, g, rl = H.case(name)
        nzd, gd = torch.as_tensor(nz, device="cuda"), torch.as_tensor(g, device="cuda")
        want_y, want_r, wst, _trace = H.model_step(name, lam, kind, radius)
        assert wst["flags"] == 0, (name, lam, kind, radius, wst)
        delta = H.radius_of(name, lam, kind, radius)
        for batch in ("1", "8"):
            os.environ["FDJAC_CSC_BATCH"] = batch
            s = fd.CscTrustRegion((colptr, rowval, N), idx_base=0)
            s.set_options(H.RTOL, H.MAXIT)
            y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
            r = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
            s.step(nzd, gd, y, delta, lam, "diag" if kind else "I", r_out=r)
            st = s.status()
            ok = TM.same_status(st, wst) and np.array_equal(bits(y.cpu().numpy()), bits(want_y)) and np.array_equal(bits(r.cpu().numpy()), bits(want_r))
            print("%s lam %g kind %d radius %s batch %s: %s exit %d iterations %d (model %d %d) step norm %.17g (model %.17g)"
                  % (name, lam, kind, radius, batch, "ok" if ok else "MISMATCH", st["exit"], st["iterations"], wst["exit"], wst["iterations"],
                     st["step_norm"], wst["step_norm"]), flush=True)
            failures += 0 if ok else 1
    if failures:
        print("%d mismatches" % failures)
        return 1
    print("all ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
