"""Wall time of the published clouds' way out (LidarOdometryServer.cpp:240-263 PublishClouds: EigenToPointCloud2, RosUtils.cpp:40-63,
of the frame, the keypoints and the local map) through the drop-in, fp64 + the node's host conversion against the FLOAT32 egress
(tests/cpp/egress_facade_test, the caller bound as tools/bench_pipeline.py binds it):
  map   (a) LocalMap() + the conversion loop against (b) LocalMapF32, on the drive's final map and on a cfg2-size map (~1M points);
  drive the drive of tools/bench_pipeline.py (131 072-point raw clouds) through RegisterIngestedFrame + the three conversions, through
        RegisterIngestedFrameF32 with both outputs (+ LocalMapF32), and with both outputs null (no subscriber: nothing published).
Prints one JSON line: median and p10 / p90 of each, in ms.

    python tools/bench_egress.py [--frames 40] [--skip 5] [--big 1200000] [--reps 30]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_pipeline import placement  # noqa: E402
from tests import egress_ref as E  # noqa: E402


def parse(lines):
    out = {}
    for line in lines:
        w = line.split()
        if len(w) >= 9 and w[1] == "median":
            out[w[0]] = {"median_ms": float(w[2]), "p10_ms": float(w[4]), "p90_ms": float(w[6]), "n": int(w[8])}
        elif w and w[0] == "map_points":
            out["map_points"] = int(w[1])
            out.update({w[i]: int(w[i + 1]) for i in range(2, len(w) - 1, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--big", type=float, default=1.2e6, help="points handed to the cfg2-size map (about 80 %% are kept)")
    ap.add_argument("--deskew", type=int, default=1)
    a = ap.parse_args()
    bind, where = placement()
    harness = E.build_harness()
    ext, frames = E.cloud_drive(a.frames, beams=64, az=2048, seed=2025, small_scene=False)
    res = {"caller_process": where}
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "drive.bin")
        E.write_cloud_drive(f, ext, frames, 1.0, 100.0, 0.0, a.deskew)
        out = subprocess.check_output([harness, "timed", f, "raw", str(a.reps)], text=True, preexec_fn=bind).splitlines()
        res["drive"] = parse(out)
    out = subprocess.check_output([harness, "bigmap", str(int(a.big)), str(a.reps), "-"], text=True, preexec_fn=bind).splitlines()
    res["cfg2_size_map"] = parse(out)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
