"""See-through removal through the drop-in C++ headers (tests/cpp/view_facade_test.cpp): the pinned 8-frame drive with a person walking
through (tests/view_cases.py) through KinematicICP five times.  With a view under which nothing is in range, poses, returned clouds and
the map must be bit-identical to the feature disabled; with the drive's configuration, per-frame statistics, poses, clouds and the final
map must equal the same sequence issued frame by frame through the C-ABI (pre-steps, register, render, sweep, update); a copy of the
object made after frame 3 must end with the same map; with Config::update_map = false the removal is skipped."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kinematic_icp_amd import synthetic as syn
from mapdev_ref import bucket_sorted
import view_cases as vc

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "view_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "view_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_view_facade_compiles_and_links():
    assert os.path.exists(build_binary())


def write_drive(path, view_path, cfg=vc.DRIVE_CFG):
    """the pinned drive as the pipeline's input: the frames in the LIDAR frame (the sensor 1.7 m above the base, no rotation), the wheel
    odometry between the true poses with a small error -> the number of frames"""
    frames = vc.drive()
    ext = np.concatenate([[0.0, 0.0, 0.0, 1.0], frames[0]["sensor"]])
    with open(path, "wb") as fh:
        np.array([len(frames), vc.DRIVE_VS, vc.DRIVE_MAX_RANGE, 0.0]).tofile(fh)
        ext.tofile(fh)
        last = syn.IDENTITY
        for k, fr in enumerate(frames):
            pts = np.ascontiguousarray(fr["frame"] - fr["sensor"])
            delta = syn.pose_mul(syn.pose_mul(syn.pose_inverse(last), fr["pose"]), syn.planar_pose(0.01 * (-1) ** k, 0.0, np.deg2rad(0.1)))
            last = fr["pose"]
            np.array([float(len(pts))]).tofile(fh)
            pts.tofile(fh), np.zeros(len(pts)).tofile(fh), delta.tofile(fh)
    np.array([cfg[k] for k in ("res", "window", "min_rays", "max_ray", "margin", "margin_per_metre")], dtype=np.float64).tofile(view_path)
    return len(frames)


def _map(path):
    raw = np.fromfile(path)
    assert len(raw) == 1 + 3 * int(raw[0])
    return bucket_sorted(raw[1:].reshape(-1, 3), vc.DRIVE_VS)


@pytest.mark.gpu
def test_removal_through_the_pipeline(tmp_path):
    f, g, prefix = tmp_path / "pipe.bin", tmp_path / "view.bin", str(tmp_path / "out")
    n = write_drive(f, g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    print("\n".join(out))
    stats = {}
    for ln in out:
        w = ln.split()
        if len(w) == 6:
            stats.setdefault(w[0], {})[int(w[1])] = tuple(int(v) for v in w[2:])
    assert "plain_has_no_view 1" in out and "copy_has_its_own_view 1" in out and "frames_rendered %d" % n in out and "disabled 1 0" in out

    # nothing in range: poses, returned clouds and the map are those of the feature disabled
    assert open(prefix + "_plain.bin", "rb").read() == open(prefix + "_tiny.bin", "rb").read()
    plain = _map(prefix + "_plain_map.bin")
    assert np.array_equal(_map(prefix + "_tiny_map.bin"), plain)
    assert stats["tiny"] == {k: (0, 0, 0, 0) for k in range(n)}

    # the drive's configuration: the same as the sequence issued through the C-ABI, frame by frame
    assert stats["on"] == stats["manual"] and sorted(stats["on"]) == list(range(n))
    assert open(prefix + "_on.bin", "rb").read() == open(prefix + "_manual.bin", "rb").read()
    on = _map(prefix + "_on_map.bin")
    assert np.array_equal(on, _map(prefix + "_manual_map.bin"))
    removed = sum(s[1] for s in stats["on"].values())
    assert stats["on"][0] == (0, 0, 0, 0)  # the first frame meets an empty map
    assert removed > 0 and all(stats["on"][k][0] > 0 for k in range(1, n)) and len(on) < len(plain)
    # the person's trail: map points above the ground within 0.4 m of the places the person stood in frames 0 .. 5 (nothing else is there);
    # the figures are printed, the equalities above are the check
    frames = vc.drive()

    def trail(cloud):
        near = np.zeros(len(cloud), dtype=bool)
        for fr in frames[:6]:
            centre = fr["person"][:, :2].mean(axis=0)
            near |= (np.linalg.norm(cloud[:, :2] - centre, axis=1) < 0.4) & (cloud[:, 2] > 0.3)
        return int(near.sum())
    print("trail: %d points without removal, %d with; removed %d in all" % (trail(plain), trail(on), removed))
    assert trail(on) < trail(plain)

    # a copy made after frame 3 went on with the same frames: the same statistics and the same map
    assert stats["copy"] == {k: stats["on"][k] for k in range(4, n)}
    assert np.array_equal(_map(prefix + "_copy_map.bin"), on)

    # update_map = false: the map is a prior, the removal is skipped
    assert stats["prior"] == {k: (0, 0, 0, 0) for k in range(4, n)} and "prior_frames_rendered 0" in out
    assert np.array_equal(_map(prefix + "_prior_map.bin"), _map(prefix + "_prior_before_map.bin"))
