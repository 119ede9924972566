"""bench.py's plain run: the contract's line with --steps honoured, nothing of --full in it, and --dump-outputs giving what the last
timed step returned - the same arrays from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

B = 96  # scans per step; the 8 distinct scans of cfg1 are cycled, so scan i of a step is scan i % 8


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--scans-per-step", str(B),
           "--workload", "cfg1", "--scans", "8", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-6000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    runs = [_run(tmp_path / "a"), _run(tmp_path / "b")]
    for out in runs:
        assert out["steps"] == 3 and out["warmup"] == 1 and out["config"]["scans_per_step"] == B
        assert out["unit"] == "scans/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
        assert out["value"] > 0 and out["ms_per_step"] > 0
        assert abs(out["value"] * out["ms_per_step"] / 1e3 - B) < 1e-3 * B  # value = scans per step / time per step
        assert "roofline" not in out and "cpu_baseline" not in out and "value_one_scan_in_flight" not in out  # (--full only)
    poses = [np.load(tmp_path / d / "poses.npy") for d in ("a", "b")]
    iters = [np.load(tmp_path / d / "iterations.npy") for d in ("a", "b")]
    for p, it in zip(poses, iters):
        assert p.dtype == np.float64 and p.shape == (B, 7) and np.all(np.isfinite(p))
        assert it.dtype == np.float64 and it.shape == (B,) and np.all(it >= 1)
        np.testing.assert_array_equal(p[8:], p[:-8])  # the same scan, the same pose, wherever it sits in the batch
    np.testing.assert_array_equal(poses[0], poses[1])
    np.testing.assert_array_equal(iters[0], iters[1])
