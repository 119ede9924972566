"""The occupancy grid through the drop-in C++ headers (tests/cpp/grid_facade_test.cpp): the six-frame drive of tests/test_facade.py's
pipeline test through KinematicICP twice, with EnableGrid and without.  Poses and returned clouds must be bit-equal between the two
runs; the grid must equal the Python mirror integrating the returned frames at the returned poses; a copy of the object made after
frame 3 must end with the same grid as the original; SaveGrid must write both files."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
from kinematic_icp_amd import synthetic as syn
import grid_ref as gr

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "grid_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "grid_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_grid_facade_compiles_and_links():
    assert os.path.exists(build_binary())


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
def test_grid_through_the_pipeline(tmp_path):
    # the drive of tests/test_facade.py::test_facade_pipeline_matches_oracle_pipeline (deskew on)
    rng = np.random.Generator(np.random.PCG64(77))
    scene = syn.make_scene(rng, half=16.0, height=4.0, n_boxes=6, box_xy=(2.0, 5.0), box_z=(1.5, 3.5), keep_clear=3.0)
    dirs = syn.beam_directions(12, 512, (-20.0, 8.0))
    ext = np.concatenate([[0, 0, np.sin(0.05), np.cos(0.05)], [0.3, 0.0, 0.9]])  # lidar_to_base
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
    f, g, prefix = tmp_path / "pipe.bin", tmp_path / "grid.bin", str(tmp_path / "out")
    with open(f, "wb") as fh:
        np.array([len(frames), voxel, max_range, float(deskew)]).tofile(fh)
        ext.tofile(fh)
        for fr, st, dl in zip(frames, stamps, deltas):
            np.array([float(len(fr))]).tofile(fh)
            np.ascontiguousarray(fr).tofile(fh), st.tofile(fh), dl.tofile(fh)
    cfg = gr.make_config(0.1, -20.0, -20.0, 400, 400, 0.3, 1.6, 25.0)  # the 32 m scene with a margin; reach 250 cells
    np.array([cfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_min", "z_max", "max_ray")], dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    assert "refused_without_grid 1 0" in out and "copy_has_its_own_grid 1" in out and "frames_integrated 6" in out and "disabled 1" in out

    # poses and returned clouds: bit-equal with and without the grid
    assert open(prefix + "_plain.bin", "rb").read() == open(prefix + "_grid.bin", "rb").read()
    run = _read_run(prefix + "_grid.bin", 6)
    # the grid: the Python mirror integrating the returned frames at the returned poses, the sensor at lidar_to_base's translation
    grid = K.OccupancyGrid(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_min"], cfg["z_max"], cfg["max_ray"])
    want = np.zeros((400, 400, 2), dtype=np.uint16)
    for pose, frame, _ in run:
        stats = grid.integrate(frame, pose, ext[4:])
        assert stats == gr.integrate(cfg, want, frame, pose, ext[4:]) and stats[0] > 500 and stats[3] > 5000
    counts = np.fromfile(prefix + "_counts.bin", dtype=np.uint16).reshape(400, 400, 2)
    assert np.array_equal(counts, grid.counts()) and np.array_equal(counts, want)
    assert counts[:, :, 1].max() == 6  # the cells around the robot were carved by every frame
    # a copy made after frame 3 went on with the same frames: the same grid
    assert np.array_equal(np.fromfile(prefix + "_copy_counts.bin", dtype=np.uint16).reshape(400, 400, 2), counts)
    occ = np.fromfile(prefix + "_occupancy.bin", dtype=np.int8).reshape(400, 400)
    assert np.array_equal(occ, gr.occupancy(counts, 2))
    pgm, yaml = gr.map_files(prefix + "_map", occ, cfg["cell"], cfg["origin_x"], cfg["origin_y"])
    assert open(prefix + "_map.pgm", "rb").read() == pgm and open(prefix + "_map.yaml").read() == yaml
