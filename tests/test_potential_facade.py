"""The cost-to-go field and its path through the drop-in C++ headers (tests/cpp/potential_facade_test.cpp): a short drive through
KinematicICP with a grid, then GridPotential towards the cell the drive started in, GridPotentialOfCostmap over GridCostmap's bytes
and PotentialPath from the cell the robot ended in.  Everything must equal the restatement (tests/potential_ref.py) over the numpy
costmap of the drive's counters."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kinematic_icp_amd import synthetic as syn
import clearance_ref as cr
import grid_ref as gr
import potential_ref as pr

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "potential_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "potential_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_potential_facade_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_potential_through_the_pipeline(tmp_path):
    # four frames of the drive of tests/test_clearance_facade.py, on 300 x 300 cells of 0.1 m
    rng = np.random.Generator(np.random.PCG64(77))
    scene = syn.make_scene(rng, half=16.0, height=4.0, n_boxes=6, box_xy=(2.0, 5.0), box_z=(1.5, 3.5), keep_clear=3.0)
    dirs = syn.beam_directions(12, 512, (-20.0, 8.0))
    ext = np.concatenate([[0, 0, np.sin(0.05), np.cos(0.05)], [0.3, 0.0, 0.9]])  # lidar_to_base
    n_frames, radius, max_potential = 4, 5, 4000
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
    cfg = gr.make_config(0.1, -5.0, -20.0, 300, 300, 0.3, 1.6, 8.0)
    W, H = cfg["width"], cfg["height"]
    goals = [(50, 200), (299, 0), (50, 200)]  # the cell of the world's origin, where the drive began, twice, and a far corner
    np.array([cfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_min", "z_max", "max_ray")] + [radius, 0.35, 3.0, max_potential, len(goals)] +
             [v for goal in goals for v in goal], dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    assert "refused_without_grid 1 1 1" in out and "refused_goal_outside_the_grid 1" in out and "refused_unreachable_start 1" in out
    assert "refused_costmap_of_another_size 1" in out

    import kinematic_icp_amd as K
    counts = np.fromfile(prefix + "_counts.bin", dtype=np.uint16).reshape(H, W, 2)
    occ = gr.occupancy(counts)
    table = K.nav2_cost_table(cfg["cell"], radius, 0.35, 3.0)
    costmap = cr.costmap(occ, table, inflate_unknown=True, clear=cr.clearance_by_offsets(occ, radius))
    assert np.array_equal(np.fromfile(prefix + "_costmap.bin", dtype=np.uint8).reshape(H, W), costmap)
    weight = pr.weights(unknown_weight=120)  # the program's: NavFn's numbers, and unknown space passable at a price
    want, want_stats = pr.potential_dijkstra(costmap, weight, goals)
    assert want_stats[0] >= 2 and want_stats[1] > 1000 and (want == pr.UNREACHED).sum() > 100  # lethal and inscribed cells are not entered
    potential = np.fromfile(prefix + "_potential.bin", dtype=np.uint32).reshape(H, W)
    assert np.array_equal(potential, want)
    assert np.array_equal(np.fromfile(prefix + "_of_costmap.bin", dtype=np.uint32).reshape(H, W), want)
    clamped, clamped_stats = pr.potential_dijkstra(costmap, weight, goals, max_potential)
    assert clamped_stats[2] > 100 and clamped_stats[1] > 100
    assert np.array_equal(np.fromfile(prefix + "_clamped.bin", dtype=np.uint32).reshape(H, W), clamped)
    stats = np.fromfile(prefix + "_stats.bin", dtype=np.uint64).reshape(3, 4)
    assert tuple(stats[0, :3].tolist()) == want_stats == tuple(stats[1, :3].tolist()) and tuple(stats[2, :3].tolist()) == clamped_stats and (stats[:, 3] >= 1).all()
    pose = np.fromfile(prefix + "_pose.bin")
    start = (int(np.floor((pose[4] + 5.0) / 0.1)), int(np.floor((pose[5] + 20.0) / 0.1)))
    path = [tuple(c) for c in np.fromfile(prefix + "_path.bin", dtype=np.uint32).reshape(-1, 2).tolist()]
    assert path == pr.path(want, costmap, weight, start) and path[0] == start and path[-1] == (50, 200) and len(path) >= 8
