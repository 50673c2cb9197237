"""bench.py's plain run and --dump-outputs on the GPU: a plain line carries the headline fields only, and two runs with the same arguments
write the same files with the same values (whichever launch mode the auto pilot picks in each run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--prime", "2", "--grid", "64", "--pts", "16384"]


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_runs_dump_the_same_outputs(tmp_path):
    lines = [_bench(tmp_path / k) for k in ("a", "b")]
    for d in lines:
        assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
        assert d["roofline"] is None and d["work_per_step"] is None and "cpu_baseline" not in d and "extras" not in d
        assert d["launch_modes"]["timed"] in ("eager_three_streams", "hipgraph_replay")
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "loss_vel.npy", "regularizers.npy", "rgb_render0.npy", "rgb_render1.npy", "param_00.npy", "adam_exp_avg_00.npy"} <= set(files)
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and a.shape == b.shape, f
        total += a.nbytes
        assert np.isfinite(a).all(), f
        peak = float(np.abs(b).max()) + 1e-30
        d = np.abs(a.astype(np.float64) - b)
        # the same iteration from the same inputs: equal up to the order of the atomic gradient sums
        assert float(np.mean(d > 1e-4 * peak)) <= 1e-3, (f, float(d.max()) / peak)
    assert total <= 64 << 20
    print("launch modes timed:", [d["launch_modes"]["timed"] for d in lines])
