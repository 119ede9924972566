"""Whole-frame timing of the 2-D LiDAR mode (online_node.cpp:44-58) through the drop-in KinematicICP, two ways, in one process, on
the same frames of a synthetic cfg4 drive, alternating frame by frame (tests/cpp/laserscan_facade_test scan_timed):
  (a) IngestScan + RegisterIngestedFrame: the raw LaserScan ranges (4 bytes per beam) go to the GPU and are projected there;
  (b) the projection on the host by the same recalled laser_geometry rules into 16-byte PointCloud2 records (C++, in the clock),
      then IngestCloud + RegisterIngestedFrame - what a node does today.
Prints one JSON line: the median and the 10th / 90th percentiles of either, over the frames after the first `--skip`.

    python tools/bench_laserscan.py [--frames 200] [--skip 20] [--deskew 1]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kinematic_icp_amd import synthetic as syn  # noqa: E402
from tests import laserscan_ref as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--skip", type=int, default=20)
    ap.add_argument("--deskew", type=int, default=1)
    a = ap.parse_args()
    cfg = syn.CONFIGS["cfg4"]
    params, ext, frames = syn.make_laser_drive(a.frames)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "scan.bin")
        L.write_drive(f, params, ext, frames, cfg.voxel_size, cfg.max_range, 0.0, a.deskew)
        out = subprocess.check_output([L.build_harness(), "scan_timed", f], text=True).splitlines()
    rows = [l.split() for l in out if l.startswith("frame")]
    ms_a = np.array([float(r[3]) for r in rows])[a.skip:]
    ms_b = np.array([float(r[5]) for r in rows])[a.skip:]
    pa = [l.split()[1:] for l in out if l.startswith("pose_a")]
    pb = [l.split()[1:] for l in out if l.startswith("pose_b")]
    stat = lambda x: {"median_ms": round(float(np.median(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4),  # noqa: E731
                      "p90_ms": round(float(np.percentile(x, 90)), 4)}
    print(json.dumps({"frames_timed": int(ms_a.size), "beams": int(frames[0]["ranges"].size), "deskew": bool(a.deskew),
                      "a_ingest_scan": stat(ms_a), "b_host_projection_ingest_cloud": stat(ms_b),
                      "same_poses": pa == pb, "map_points": out[-1].split()[1:]}))


if __name__ == "__main__":
    main()
