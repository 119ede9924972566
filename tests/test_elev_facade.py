"""The height columns through the drop-in C++ headers (tests/cpp/elev_facade_test.cpp): the six-frame drive of tests/test_facade.py's
pipeline test through KinematicICP twice, with EnableElevation and without.  Poses and returned clouds must be bit-equal between the
two runs; the layer must equal the Python mirror integrating the returned frames at the returned poses, statistics and window
included; a copy of the object made after frame 3 must end with the same layer; ElevationTraversability must equal the mirror's."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
from kinematic_icp_amd import synthetic as syn
import clearance_ref as cr
import elev_cases as ec
import elev_ref as er

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "elev_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "elev_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_elev_facade_compiles_and_links():
    assert os.path.exists(build_binary())


def write_drive(path):
    """the drive of tests/test_facade.py::test_facade_pipeline_matches_oracle_pipeline (deskew on), as tests/test_grid_facade.py writes
    it -> lidar_to_base"""
    rng, scene, dirs = ec.drive_scene()
    ext = ec.DRIVE_EXT
    voxel, max_range, deskew = 0.5, 30.0, 1
    poses, frames, stamps, deltas = [syn.planar_pose(0.0, 0.0, 0.1)], [], [], []
    for k in range(6):
        delta_true = syn.planar_pose(0.25, 0.0, np.deg2rad(2.0 + k))
        poses.append(syn.pose_mul(poses[-1], delta_true))
        world_from_lidar = syn.pose_mul(poses[-1], ext)
        R = syn.quat_to_matrix(world_from_lidar[:4])
        t = scene.raycast(world_from_lidar[4:], dirs @ R.T) + rng.normal(0, 0.01, len(dirs))
        frames.append(dirs * t[:, None])
        stamps.append(np.linspace(0.0, 1.0, len(dirs)))
        deltas.append(syn.pose_mul(delta_true, syn.planar_pose(0.01 * (-1) ** k, 0.0, np.deg2rad(0.15))))
    with open(path, "wb") as fh:
        np.array([len(frames), voxel, max_range, float(deskew)]).tofile(fh)
        ext.tofile(fh)
        for fr, st, dl in zip(frames, stamps, deltas):
            np.array([float(len(fr))]).tofile(fh)
            np.ascontiguousarray(fr).tofile(fh), st.tofile(fh), dl.tofile(fh)
    return ext


def _read_run(path, n_frames):
    raw = np.fromfile(path)
    frames, at = [], 0
    for _ in range(n_frames):
        pose = raw[at:at + 7]
        at += 7
        clouds = []
        for _ in range(2):
            n = int(raw[at])
            clouds.append(raw[at + 1:at + 1 + 3 * n].reshape(n, 3))
            at += 1 + 3 * n
        frames.append((pose, clouds[0], clouds[1]))
    assert at == len(raw)
    return frames


@pytest.mark.gpu
def test_elevation_through_the_pipeline(tmp_path):
    f, g, prefix = tmp_path / "pipe.bin", tmp_path / "layer.bin", str(tmp_path / "out")
    ext = write_drive(f)
    cfg = er.make_config(0.1, -14.0, -14.0, 300, 300, -1.0, 0.0625, 12.0)  # tests/elev_cases.py's drive layer: walls outside, the ceiling above
    S, H = 2, 24
    np.array([cfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_origin", "slab", "max_ray")] + [S, H], dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    assert "refused_without_layer 1 0" in out and "copy_has_its_own_layer 1" in out and "frames_integrated 6" in out and "disabled 1" in out

    # poses and returned clouds: bit-equal with and without the layer
    assert open(prefix + "_plain.bin", "rb").read() == open(prefix + "_elev.bin", "rb").read()
    run = _read_run(prefix + "_elev.bin", 6)
    # the layer: the Python mirror integrating the returned frames at the returned poses, the sensor at lidar_to_base's translation
    layer = K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_origin"], cfg["slab"], cfg["max_ray"])
    want = np.zeros((300, 300), dtype=np.uint64)
    got_stats = [tuple(int(v) for v in ln.split()[2:]) for ln in out if ln.startswith("stats ")]
    for k, (pose, frame, _) in enumerate(run):
        stats = layer.integrate(frame, pose, ext[4:])
        assert stats == er.integrate(cfg, want, frame, pose, ext[4:]) == got_stats[k] and stats[0] > 1000 and stats[4] > 100
    columns = np.fromfile(prefix + "_columns.bin", dtype=np.uint64).reshape(300, 300)
    assert np.array_equal(columns, layer.columns()) and np.array_equal(columns, want)
    # a copy made after frame 3 went on with the same frames: the same layer
    assert np.array_equal(np.fromfile(prefix + "_copy_columns.bin", dtype=np.uint64).reshape(300, 300), columns)
    # ElevationTraversability, ElevationLastWindow: the mirror's
    classes, ground, counts = layer.traversability(S, H, return_ground=True, return_counts=True)
    raw = np.fromfile(prefix + "_classes.bin", dtype=np.uint8)
    assert np.array_equal(raw[:90000].view(np.int8).reshape(300, 300), classes) and np.array_equal(raw[90000:].reshape(300, 300), ground)
    assert ("counts %d %d %d %d" % counts) in out and counts[1] > 1000 and counts[2] > 100
    window = layer.last_window()
    assert ("window %d %d %d %d" % window) in out and window == er.window(cfg, run[-1][0], ext[4:])
    x0, y0, w, h = cr.grown(window, 1, 300, 300)
    assert np.array_equal(np.fromfile(prefix + "_window.bin", dtype=np.int8).reshape(h, w), classes[y0:y0 + h, x0:x0 + w])
