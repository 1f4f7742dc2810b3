"""bench.py's two kinds of run: a plain one (set-up, warm-up, the K timed steps, the headline line) and --full (everything else
it measures and checks); --dump-outputs writes the nzval of the last timed step, whole or as a fixed sample above 64 MB."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_below_the_cap_and_a_fixed_sample_above(tmp_path):
    torch = pytest.importorskip("torch")
    B = _bench_module()
    small = torch.arange(1000, dtype=torch.float32)
    B.dump_outputs(str(tmp_path), "small", small)
    got = np.load(tmp_path / "small.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy())
    # an array whose entries are their own positions: the sample is then the list of positions it took
    n = B.DUMP_MAX_BYTES // 8 + 12345
    big = torch.arange(n, dtype=torch.float64)
    for name in ("a", "b"):
        B.dump_outputs(str(tmp_path / name), "big", big)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float64 and np.array_equal(a, b)                      # the same positions every time
    assert os.path.getsize(tmp_path / "a" / "big.npy") <= B.DUMP_MAX_BYTES
    assert np.all(np.diff(a) > 0) and a.size > B.DUMP_SAMPLE // 2
    edge = B.DUMP_EDGE
    assert np.array_equal(a[:edge], np.arange(edge)) and np.array_equal(a[-edge:], np.arange(n - edge, n))


def _run(args, timeout):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_plain_run_is_the_headline_only_and_dumps_what_full_computes(tmp_path):
    N = 300001
    common = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--size", str(N)]
    plain = _run(common + ["--dump-outputs", str(tmp_path / "plain")], 180)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 7 and plain["ms_per_step"] > 0 and plain["dtype"] == "f64"
    assert abs(plain["value"] - N / (plain["ms_per_step"] * 1e-3)) <= 1e-9 * plain["value"]
    assert not any(k in plain for k in ("roofline", "result_check", "cpu_baseline", "rotating_x", "rank_share"))
    nz = np.load(tmp_path / "plain" / "nzval.npy")
    assert nz.dtype == np.float64 and nz.shape == (3 * N - 2,)
    exact = np.where(np.arange(nz.size) % 3 == 0, -2.0, 1.0)                # CSC order: (du, d, dl) per column, column 0 = (d, dl)
    assert np.max(np.abs(nz - exact)) < 1e-6
    full = _run(common + ["--full", "--no-cpu-baseline", "--no-plain-handover", "--soak-seconds", "0",
                          "--dump-outputs", str(tmp_path / "full")], 300)
    assert full["result_check"]["ok"] and full["roofline"]["kernel"] and full["median_ms_per_step"] > 0
    assert {k: full[k] for k in plain if k not in ("value", "ms_per_step")} == {k: v for k, v in plain.items() if k not in ("value", "ms_per_step")}
    assert np.array_equal(np.load(tmp_path / "full" / "nzval.npy"), nz)     # the same bits either way
