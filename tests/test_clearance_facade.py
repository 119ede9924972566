"""The grid's clearance and costmap through the drop-in C++ headers (tests/cpp/clearance_facade_test.cpp): a short drive through
KinematicICP with a grid; after every frame the program refreshes its costmap in GridLastWindow() grown by the radius only.  That
costmap must equal the full one; the full costmap and clearance must equal the numpy restatement over the drive's counters; every
window must be the one the restatement derives from the frame's pose."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kinematic_icp_amd import synthetic as syn
import clearance_ref as cr
import grid_ref as gr

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "clearance_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "clearance_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_clearance_facade_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_costmap_through_the_pipeline(tmp_path):
    # four frames of the drive of tests/test_grid_facade.py, on 300 x 300 cells of 0.1 m whose left edge clips the windows
    rng = np.random.Generator(np.random.PCG64(77))
    scene = syn.make_scene(rng, half=16.0, height=4.0, n_boxes=6, box_xy=(2.0, 5.0), box_z=(1.5, 3.5), keep_clear=3.0)
    dirs = syn.beam_directions(12, 512, (-20.0, 8.0))
    ext = np.concatenate([[0, 0, np.sin(0.05), np.cos(0.05)], [0.3, 0.0, 0.9]])  # lidar_to_base
    n_frames, radius = 4, 10
    poses = [syn.planar_pose(0.0, 0.0, 0.1)]
    f, g, prefix = tmp_path / "pipe.bin", tmp_path / "grid.bin", str(tmp_path / "out")
    with open(f, "wb") as fh:
        np.array([n_frames, 0.5, 30.0, 1.0]).tofile(fh)
        ext.tofile(fh)
        for k in range(n_frames):
            delta_true = syn.planar_pose(0.25, 0.0, np.deg2rad(2.0 + k))
            poses.append(syn.pose_mul(poses[-1], delta_true))
            world_from_lidar = syn.pose_mul(poses[-1], ext)
            t = scene.raycast(world_from_lidar[4:], dirs @ syn.quat_to_matrix(world_from_lidar[:4]).T) + rng.normal(0, 0.01, len(dirs))
            np.array([float(len(dirs))]).tofile(fh)
            np.ascontiguousarray(dirs * t[:, None]).tofile(fh), np.linspace(0.0, 1.0, len(dirs)).tofile(fh)
            syn.pose_mul(delta_true, syn.planar_pose(0.01 * (-1) ** k, 0.0, np.deg2rad(0.15))).tofile(fh)
    cfg = gr.make_config(0.1, -5.0, -20.0, 300, 300, 0.3, 1.6, 8.0)  # reach 80 cells: the windows are clipped at the grid's left edge
    W, H = cfg["width"], cfg["height"]
    np.array([cfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_min", "z_max", "max_ray")] + [radius, 0.35, 3.0], dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    assert "refused_without_grid 1 1 1" in out and "window_before_any_frame_is_empty 1" in out and "refused_outside_the_grid 1" in out

    import kinematic_icp_amd as K
    table = np.fromfile(prefix + "_table.bin", dtype=np.uint8)
    assert np.array_equal(table, K.nav2_cost_table(cfg["cell"], radius, 0.35, 3.0))
    run_poses = np.fromfile(prefix + "_poses.bin").reshape(n_frames, 7)
    windows = np.fromfile(prefix + "_windows.bin", dtype=np.uint32).reshape(n_frames, 4)
    for pose, window in zip(run_poses, windows):
        assert tuple(int(v) for v in window) == cr.window(cfg, pose, ext[4:])
    assert (windows[:, 2] < 2 * cfg["reach"] + 1).all() and (windows[:, 3] == 2 * cfg["reach"] + 1).all()  # clipped in x only
    counts = np.fromfile(prefix + "_counts.bin", dtype=np.uint16).reshape(H, W, 2)
    occ = gr.occupancy(counts)
    assert (occ > 65).sum() > 100 and (occ == 0).sum() > 1000 and (occ == -1).sum() > 1000  # the drive drew something of every class
    clear = cr.clearance_by_offsets(occ, radius)
    assert np.array_equal(np.fromfile(prefix + "_clearance.bin", dtype=np.uint16).reshape(H, W), clear)
    full = np.fromfile(prefix + "_costmap.bin", dtype=np.uint8).reshape(H, W)
    assert np.array_equal(full, cr.costmap(occ, table, inflate_unknown=True, clear=clear))
    assert np.array_equal(np.fromfile(prefix + "_kept.bin", dtype=np.uint8).reshape(H, W), full)  # refreshing the grown windows was enough
    x0, y0, w, h = cr.grown(tuple(int(v) for v in windows[-1]), radius, W, H)
    assert np.array_equal(np.fromfile(prefix + "_patch.bin", dtype=np.uint16).reshape(h, w), clear[y0:y0 + h, x0:x0 + w])
