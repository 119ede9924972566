"""Helpers of the egress tests and tools/bench_egress.py: the drives of tests/cpp/egress_facade_test (the published clouds as
PointCloud2 `data`, RosUtils.cpp:40-63 EigenToPointCloud2, LidarOdometryServer.cpp:240-263 PublishClouds) and the harness itself."""
import os
import subprocess

import numpy as np

from kinematic_icp_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "build", "egress_facade_test")


def build_harness():
    """tests/cpp/egress_facade_test against the drop-in headers and libkicp_amd.so, built under build/ (rebuilt when a source is newer)."""
    cpp = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
    src = os.path.join(ROOT, "tests", "cpp", "egress_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(cpp) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(HARNESS) or any(os.path.getmtime(d) > os.path.getmtime(HARNESS) for d in deps):
        os.makedirs(os.path.dirname(HARNESS), exist_ok=True)
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        tmp = HARNESS + ".%d" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", cpp, "-I", os.path.join(cpp, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", tmp, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
        os.replace(tmp, HARNESS)
    return HARNESS


def narrow(xyz):
    """static_cast<float> of every double, as uint32 words: what EigenToPointCloud2 writes, compared bit for bit"""
    with np.errstate(over="ignore"):  # (beyond the float range: +-inf, as static_cast<float>)
        return np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3).astype(np.float32)).view(np.uint32)


def cloud_drive(n_frames, beams=12, az=512, seed=77, small_scene=True):
    """A drive of raycast clouds as PointCloud2 carries them (x y z t FLOAT32): (lidar_to_base, [(records (n, 4) float32, delta)])"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if small_scene:
        scene = syn.make_scene(rng, half=16.0, height=4.0, n_boxes=6, box_xy=(2.0, 5.0), box_z=(1.5, 3.5), keep_clear=3.0)
        dirs, step = syn.beam_directions(beams, az, (-20.0, 8.0)), 0.25
    else:  # the scene and drive of tools/bench_pipeline.py
        scene, dirs, step = syn.make_scene(rng), syn.beam_directions(beams, az), 0.5
    ext = np.concatenate([[0, 0, np.sin(0.05), np.cos(0.05)], [0.3, 0.0, 0.9 if small_scene else 1.8]])
    pose, out = syn.planar_pose(0.0, 0.0, 0.1), []
    for k in range(n_frames):
        delta_true = syn.planar_pose(step, 0.0, np.deg2rad(2.0 + 0.1 * k))
        pose = syn.pose_mul(pose, delta_true)
        wl = syn.pose_mul(pose, ext)
        t = scene.raycast(wl[4:], dirs @ syn.quat_to_matrix(wl[:4]).T) + rng.normal(0, 0.01, len(dirs))
        rec = np.empty((len(dirs), 4), dtype=np.float32)
        rec[:, :3] = dirs * t[:, None]
        rec[:, 3] = np.linspace(0.0, 0.1, len(dirs))
        out.append((rec, syn.pose_mul(delta_true, syn.planar_pose(0.01 * (-1) ** k, 0.0, np.deg2rad(0.15)))))
    return ext, out


def write_cloud_drive(path, ext, frames, voxel, max_range, min_range, deskew):
    """The input file of the harness for a cloud drive (layout: tests/cpp/egress_facade_test.cpp)"""
    with open(path, "wb") as fh:
        np.array([0.0, len(frames), voxel, max_range, min_range, float(deskew)]).tofile(fh)
        np.asarray(ext, dtype=np.float64).tofile(fh)
        for rec, delta in frames:
            np.array([float(len(rec))]).tofile(fh)
            np.ascontiguousarray(rec, dtype=np.float32).tofile(fh)
            np.asarray(delta, dtype=np.float64).tofile(fh)


def write_scan_drive(path, params, ext, frames, voxel, max_range, min_range, deskew):
    """... and for a LaserScan drive (frames of kinematic_icp_amd.synthetic.make_laser_drive)"""
    with open(path, "wb") as fh:
        np.array([1.0, len(frames), voxel, max_range, min_range, float(deskew)]).tofile(fh)
        np.asarray(ext, dtype=np.float64).tofile(fh)
        np.array([params[k] for k in ("angle_min", "angle_max", "angle_increment", "range_min", "range_max")]).tofile(fh)
        for fr in frames:
            r = np.ascontiguousarray(fr["ranges"], dtype=np.float32)
            np.array([float(r.size), fr.get("time_increment", params["time_increment"])]).tofile(fh)
            r.tofile(fh)
            np.asarray(fr["rel_odom"], dtype=np.float64).tofile(fh)


def read_map_dump(path):
    """the harness's DUMP file: per frame the LocalMapF32 records as (n, 3) uint32 words"""
    raw, out, at = open(path, "rb").read(), [], 0
    while at < len(raw):
        n = int(np.frombuffer(raw, dtype=np.uint64, count=1, offset=at)[0])
        out.append(np.frombuffer(raw, dtype=np.uint32, count=3 * n, offset=at + 8).reshape(n, 3))
        at += 8 + 12 * n
    return out
