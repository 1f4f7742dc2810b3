"""Child process of tests/test_gpu_jftr.py (not a test file): the cases of tests/jftr_cases.py SWITCHED -- the large kernels at N = 1, 2, 3,
257 and 1025 under FDJAC_SMALL=0, and k_tr_p with the JVP's own dot in place of k_jt_p under FDJAC_JFTR_FUSE=0 -- y, r_out, the exit
kind, the flags, the iteration count, the four status scalars and the counts BIT FOR BIT against tests/jftr_model.py.  The parent starts
it with FDJAC_TEST_SWITCHES=1 (the library reads its switches only then, at fd_jftr_create); it prints one line per case and "all ok" at
the end, and exits non-zero on a mismatch."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import finitediff_jl_amd as fd                # noqa: E402
import csc_tr_model as TM                     # noqa: E402
import jftr_cases as K                        # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def dev(a, off):
    """a on the device, starting on a pair (off = 0) or one element past one."""
    buf = torch.zeros(a.size + 2, dtype=torch.float64, device="cuda")
    view = buf[off:off + a.size]
    view.copy_(torch.as_tensor(np.ascontiguousarray(a), device="cuda"))
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return view


def main():
    assert os.environ.get("FDJAC_TEST_SWITCHES") == "1"
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    failures = 0
    for case in K.SWITCHED:
        os.environ["FDJAC_SMALL"] = "0" if case["small_off"] else "1"
        os.environ["FDJAC_JFTR_FUSE"] = "1" if case["fuse"] else "0"
        f0, x, g, m = K.operands(case)
        N = x.size
        cnt = {}
        want_y, want_r, wst = K.model(case, num_cus, counts=cnt)
        f = fd.BuiltinF(case["family"], *case["prm"])
        s = fd.JfTrustRegion(N, case["fdtype"])
        s.set_lazy(f if case["route"] != "plain" else None, quotient=case["route"] == "quot")
        s.set_options(case["rtol"], case["maxit"])
        s.set_policy(True)
        xd, gd, md = dev(x, case["xoff"]), dev(g, 0), dev(m, case["moff"])
        s.set_diagonal(md if case["diag"] else None)
        y = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        r = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
        s.step(f, xd, gd, y, K.radius_of(case, num_cus), case["lam"], case["beta"], r_out=r)
        st = s.status()
        apps, base = s.counts()
        ok = (TM.same_status(st, wst) and np.array_equal(bits(y.cpu().numpy()), bits(want_y)) and np.array_equal(bits(r.cpu().numpy()), bits(want_r))
              and apps == cnt["applications"] and base == (1 if case["fdtype"] == "forward" else 0))
        print("%s: %s exit %d iterations %d (model %d %d) step norm %.17g (model %.17g) applications %d (model %d)"
              % (case["id"], "ok" if ok else "MISMATCH", st["exit"], st["iterations"], wst["exit"], wst["iterations"], st["step_norm"],
                 wst["step_norm"], apps, cnt["applications"]), flush=True)
        failures += 0 if ok else 1
    if failures:
        print("%d mismatches" % failures)
        return 1
    print("all ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
