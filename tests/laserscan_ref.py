"""Test-side restatement of the 2-D LaserScan ingest (kicp_pre_ingest_scan, include/kicp.h).

laser_geometry's LaserProjection::projectLaser_ (2.x), as the 2-D mode of the node calls it (online_node.cpp:44-58:
projectLaser(*msg, cloud, -1.0, channel_option::Timestamp)).  laser_geometry is not part of the reference tree: the rules below
are RECALLED, the same ones kicp_pre_ingest.hpp (laser_rules) states for the device:
  - a cosine table C[i] = (cos a_i, sin a_i), libm double on a_i = angle_min + (float)i * angle_increment computed in float, cached
    per projector and rebuilt only when n, angle_min or angle_max changes (angle_increment is not part of the key);
  - range_cutoff < 0 -> (double)range_max; beam i kept iff r < range_cutoff (r widened to double) and r >= range_min (float);
  - x = (float)((double)r * C[i].cos), y likewise with sin, z = 0; field "stamps" = (float)i * time_increment in float, i the
    ORIGINAL beam index.
The projected cloud is packed as the 16-byte PointCloud2 records it is (x y z stamps, FLOAT32 at 0/4/8/12), so that okicp.ingest
(PointCloud2ToEigen + the FLOAT32 stamp branch of ProcessTimestamps) and the okicp pipeline take over from there.
The table uses math.cos / math.sin per beam (glibc, like the backend's host), not np.cos: a vectorised cos need not equal libm
to the last bit.
"""
import math
import os
import subprocess

import numpy as np

from oracle import okicp

F32 = np.float32
LAYOUT = (16, 0, 4, 8, 7, 12)  # point_step, offset x / y / z, FLOAT32, offset of "stamps"


class Projector:
    """One laser_geometry::LaserProjection: holds the cosine table between scans."""

    def __init__(self):
        self.table = None
        self.key = None
        self.rebuilds = 0

    def _table(self, n, angle_min, angle_max, angle_increment):
        amin, amax, inc = F32(angle_min), F32(angle_max), F32(angle_increment)
        k = self.key
        if k is None or n != k[0] or amin != k[1] or amax != k[2]:  # float compares (a NaN angle always rebuilds)
            t = np.empty((n, 2))
            for i in range(n):
                a = amin + F32(i) * inc  # float32 scalars: one rounded product, one rounded sum
                t[i, 0], t[i, 1] = math.cos(float(a)), math.sin(float(a))
            self.table, self.key = t, (n, amin, amax)
            self.rebuilds += 1
        return self.table

    def project(self, ranges, angle_min, angle_max, angle_increment, time_increment, range_min, range_max, range_cutoff=-1.0):
        """-> dict(xyz (k,3) fp64 as PointCloud2ToEigen widens them, stamps (k,) float32 raw, index (k,) original beam indices,
        packed bytes of the 16-byte records, n kept)"""
        r = np.ascontiguousarray(ranges, dtype=np.float32).ravel()
        n = r.size
        table = self._table(n, angle_min, angle_max, angle_increment)
        cutoff = float(F32(range_max)) if range_cutoff < 0 else float(range_cutoff)
        with np.errstate(invalid="ignore"):
            keep = (r.astype(np.float64) < cutoff) & (r >= F32(range_min))
        idx = np.nonzero(keep)[0]
        rk = r[idx].astype(np.float64)
        x = (rk * table[idx, 0]).astype(np.float32)
        y = (rk * table[idx, 1]).astype(np.float32)
        stamps = idx.astype(np.float32) * F32(time_increment)
        rec = np.zeros((idx.size, 4), dtype=np.float32)
        rec[:, 0], rec[:, 1], rec[:, 3] = x, y, stamps
        xyz = np.stack([x.astype(np.float64), y.astype(np.float64), np.zeros(idx.size)], axis=1)
        return dict(xyz=xyz, stamps=stamps, index=idx, packed=rec.tobytes(), n=int(idx.size))


def ingest(projected):
    """okicp.ingest of the packed records: (xyz, normalised stamps or None, (min, max) seconds) - what Ingest / IngestScan return."""
    return okicp.ingest(projected["packed"], projected["n"], *LAYOUT)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "laserscan_facade_test")


def build_harness():
    """tests/cpp/laserscan_facade_test against the drop-in headers and libkicp_amd.so (rebuilt when a source is newer)."""
    cpp = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
    src = HARNESS + ".cpp"
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(cpp) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(HARNESS) or any(os.path.getmtime(d) > os.path.getmtime(HARNESS) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", cpp, "-I", os.path.join(cpp, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", HARNESS, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return HARNESS


def write_drive(path, params, lidar_to_base, frames, voxel, max_range, min_range, deskew, range_cutoff=-1.0):
    """The input file of the harness (layout: tests/cpp/laserscan_facade_test.cpp).  A frame may carry its own time_increment."""
    with open(path, "wb") as fh:
        np.array([len(frames), voxel, max_range, min_range, float(deskew), range_cutoff]).tofile(fh)
        np.asarray(lidar_to_base, dtype=np.float64).tofile(fh)
        np.array([params[k] for k in ("angle_min", "angle_max", "angle_increment", "range_min", "range_max")]).tofile(fh)
        for fr in frames:
            r = np.ascontiguousarray(fr["ranges"], dtype=np.float32)
            np.array([float(r.size), fr.get("time_increment", params["time_increment"])]).tofile(fh)
            r.tofile(fh)
            np.asarray(fr["rel_odom"], dtype=np.float64).tofile(fh)
