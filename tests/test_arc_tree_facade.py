"""A tree of arc segments scored through the drop-in C++ headers (tests/cpp/arc_tree_facade_test.cpp): a short drive through
KinematicICP with a grid, GridPotential towards the cell the drive started in, then ScoreArcTree from the pose the robot ended at and
BestArcTreeLeaf.  ScoreArcTree must equal the C entry the program calls itself and the restatement (tests/arc_tree_ref.py) over the
plan the program's own costmap and potential give; BestArcTreeLeaf must return the restatement's leaf and path."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kinematic_icp_amd import synthetic as syn
import arcs_ref as ar
import arc_tree_ref as tr
import grid_ref as gr

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "arc_tree_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "arc_tree_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_arc_tree_facade_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_arc_tree_through_the_pipeline(tmp_path):
    # four frames of the drive of tests/test_arcs_facade.py, on 300 x 300 cells of 0.1 m
    rng = np.random.Generator(np.random.PCG64(77))
    scene = syn.make_scene(rng, half=16.0, height=4.0, n_boxes=6, box_xy=(2.0, 5.0), box_z=(1.5, 3.5), keep_clear=3.0)
    dirs = syn.beam_directions(12, 512, (-20.0, 8.0))
    ext = np.concatenate([[0, 0, np.sin(0.05), np.cos(0.05)], [0.3, 0.0, 0.9]])  # lidar_to_base
    n_frames, radius, dt = 4, 5, 0.25
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
    box = (-0.3, 0.3, -0.2, 0.2, 0.1)  # 7 x 5 samples
    branch, steps = (5, 3, 3), (4, 4, 4)  # 5 + 15 + 45 nodes: the last workgroup of every level is partial
    commands = np.array([(v, w) for v, w in [(0.6, -1.5), (0.6, -0.7), (0.6, 0.0), (0.6, 0.7), (0.6, 1.5)] + [(0.4, -1.5), (0.6, 0.0), (0.4, 1.5)] * 2])
    np.array([cfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_min", "z_max", "max_ray")] + [radius, 0.35, 3.0, 50, 200, dt] + list(box) +
             [len(branch)] + list(branch) + list(steps) + commands.ravel().tolist(), dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    for line in ("refused_without_grid 1", "refused_without_plan 1", "refused_after_a_failed_potential 1", "refused_a_tree_short_of_a_row 1", "refused_depth_9 1",
                 "counts 65 45 12"):
        assert line in out, out

    import kinematic_icp_amd as K
    costmap = np.fromfile(prefix + "_costmap.bin", dtype=np.uint8).reshape(H, W)
    potential = np.fromfile(prefix + "_potential.bin", dtype=np.uint32).reshape(H, W)
    weight = K.plan_weights(unknown_weight=120)  # the program's
    assert np.array_equal(potential, K.potential_from_costmap(costmap, weight, [(50, 200)]))
    pose, start = np.fromfile(prefix + "_pose.bin"), np.fromfile(prefix + "_start.bin")
    assert np.array_equal(start[:2], pose[4:6]) and abs(np.hypot(*start[2:]) - 1.0) < 1e-15
    primitives, footprint = np.fromfile(prefix + "_primitives.bin").reshape(-1, 4), np.fromfile(prefix + "_footprint.bin").reshape(-1, 2)
    assert np.array_equal(primitives.view(np.uint64), ar.arc_steps(commands[:, 0], commands[:, 1], dt).view(np.uint64))
    assert np.array_equal(footprint, ar.footprint_box(*box)) and len(footprint) == 35
    q = K.plan_q(costmap, weight)
    want = tr.score_tree(q, potential, cfg["cell"], cfg["origin_x"], cfg["origin_y"], start, branch, steps, primitives, footprint)
    results = np.fromfile(prefix + "_results.bin", dtype=np.uint32).reshape(-1, 4)
    print("free steps of the 45 leaves:", np.bincount(want[20:, 0], minlength=13).tolist())
    c_entry = np.fromfile(prefix + "_results_c.bin", dtype=np.uint32).reshape(-1, 4)
    assert np.array_equal(results, c_entry) and np.array_equal(results, want)  # ScoreArcTree is the C entry, and both are the header's text
    assert np.array_equal(np.fromfile(prefix + "_results_start.bin", dtype=np.uint32).reshape(-1, 4), want)
    assert np.array_equal(K.score_arc_tree_from_plan(q, potential, cfg["cell"], cfg["origin_x"], cfg["origin_y"], start, branch, steps, primitives, footprint), want)
    assert (want[20:, 0] > 4).any()  # some leaf's path went on past level 1
    best = np.fromfile(prefix + "_best.bin", dtype=np.uint64).reshape(3, 5).tolist()
    for row, rank in zip(best, ((1, 0, 0, 1), (1, 2, 300, 0), (0, 1, 0, 13))):
        expected = tr.best(want, branch, steps, *rank)
        assert row == ([0, 45] + [0xFFFFFFFF] * 3 if expected is None else [1, expected[0]] + list(expected[1])), (row, expected)
    assert best[0][0] == 1 and best[2][0] == 0  # a leaf is found, and none can have taken more than every step
    leaf, path = best[0][1], best[0][2:]
    assert leaf == (path[0] * 3 + path[1]) * 3 + path[2] and want[20 + leaf, 3] == want[20:][want[20:, 0] >= 1, 3].min()
