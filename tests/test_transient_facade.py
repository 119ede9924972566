"""The transient obstacles through the drop-in C++ headers (tests/cpp/transient_facade_test.cpp): the drive of tests/test_grid_facade.py
through KinematicICP with a grid, four frames of the room, a fifth with a box of returns standing in the space the first four carved,
and a sixth after it has left.  Transients() must equal the C entry on a second pipeline's grid and the restatement
(tests/transient_ref.py) of the returned frames at the returned poses over the restatement's counters; the costmap must be lethal on
the box's cells while the occupancy still reads them free; the frame after it must leave the costmap what the counters alone give;
poses and clouds must be bit-equal with and without EnableTransients."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
from kinematic_icp_amd import synthetic as syn
import elev_cases as ec
import grid_ref
import transient_ref as tr

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "transient_facade_test")
GRID = (0.1, -14.0, -14.0, 300, 300, 0.1, 1.5, 12.0)
PARAMS = dict(min_observations=2, free_max=25, min_points=3, min_size=3)
BOX = np.array([3.0, -2.9, 0.0, 3.4, -2.5, 1.8])  # a column of 0.4 m x 0.4 m in the wedge the first frames carve towards a box of the scene
BOX_FRAME, N_FRAMES = 4, 6


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "transient_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_transient_facade_compiles_and_links():
    assert os.path.exists(build_binary())


def write_drive(path):
    """tests/test_grid_facade.py's drive (deskew on) with the box in frame BOX_FRAME only -> lidar_to_base"""
    rng, scene, dirs = ec.drive_scene()
    with_box = syn.Scene(scene.half, scene.height, np.vstack([scene.boxes, BOX]))
    ext = ec.DRIVE_EXT
    poses, frames, stamps, deltas = [syn.planar_pose(0.0, 0.0, 0.1)], [], [], []
    for k in range(N_FRAMES):
        delta_true = syn.planar_pose(0.25, 0.0, np.deg2rad(2.0 + k))
        poses.append(syn.pose_mul(poses[-1], delta_true))
        world_from_lidar = syn.pose_mul(poses[-1], ext)
        R = syn.quat_to_matrix(world_from_lidar[:4])
        t = (with_box if k == BOX_FRAME else scene).raycast(world_from_lidar[4:], dirs @ R.T) + rng.normal(0, 0.01, len(dirs))
        frames.append(dirs * t[:, None])
        stamps.append(np.linspace(0.0, 1.0, len(dirs)))
        deltas.append(syn.pose_mul(delta_true, syn.planar_pose(0.01 * (-1) ** k, 0.0, np.deg2rad(0.15))))
    with open(path, "wb") as fh:
        np.array([len(frames), 0.5, 30.0, 1.0]).tofile(fh)
        ext.tofile(fh)
        for fr, st, dl in zip(frames, stamps, deltas):
            np.array([float(len(fr))]).tofile(fh)
            np.ascontiguousarray(fr).tofile(fh), st.tofile(fh), dl.tofile(fh)
    return ext


def read_run(path, n_frames):
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
def test_transients_through_the_pipeline(tmp_path):
    f, g, prefix = tmp_path / "pipe.bin", tmp_path / "grid.bin", str(tmp_path / "out")
    ext = write_drive(f)
    np.array(list(GRID) + [PARAMS[k] for k in ("min_observations", "free_max", "min_points", "min_size")], dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    for line in ["refused_without_grid 1", "off_by_default 1", "refused_bad_config 1", "enabled 1", "copy_carries_the_switch 1", "moved_carries_the_switch 1",
                 "counters_agree 1", "disabled 1", "enabled_without_sources 1", "new_grid_starts_off 1"] + ["same_as_the_c_entry %d 1" % k for k in range(N_FRAMES)]:
        assert line in out, line

    # poses and returned clouds: bit-equal without and with the transients
    assert open(prefix + "_off.bin", "rb").read() == open(prefix + "_on.bin", "rb").read()
    run = read_run(prefix + "_on.bin", N_FRAMES)
    cfg = grid_ref.make_config(*GRID)
    H, W = cfg["height"], cfg["width"]
    counts = np.zeros((H, W, 2), dtype=np.uint16)
    rows_raw, at = np.fromfile(prefix + "_rows.bin", dtype=np.uint64), 0
    planes = np.fromfile(prefix + "_planes.bin", dtype=np.uint8).reshape(N_FRAMES, H, W)
    table = K.nav2_cost_table(0.1, 3, 0.15, 3.0)
    # the pipeline's world is the first pose's frame, the scene's turned by -0.1 rad: the cells within 0.5 m of the box's middle there
    bx, by = (BOX[0] + BOX[3]) / 2, (BOX[1] + BOX[4]) / 2
    bx, by = bx * np.cos(0.1) + by * np.sin(0.1), -bx * np.sin(0.1) + by * np.cos(0.1)
    yy, xx = np.mgrid[0:H, 0:W]
    box_cells = np.hypot(GRID[1] + (xx + 0.5) * GRID[0] - bx, GRID[2] + (yy + 0.5) * GRID[0] - by) < 0.5
    for k, (pose, frame, _) in enumerate(run):
        want_rows, _, want_plane, stats = tr.transients(cfg, counts, frame, pose, ext[4:], **PARAMS)
        n = int(rows_raw[at])
        rows = rows_raw[at + 1:at + 1 + 10 * n].reshape(n, 10)
        at += 1 + 10 * n
        print("frame %d: %d transients %s, restatement %d, stats %s, plane %d cells" % (k, n, rows[:, 1].tolist(), len(want_rows), stats, int(want_plane.sum())))
        assert np.array_equal(rows, want_rows) and np.array_equal(planes[k], want_plane)
        grid_ref.integrate(cfg, counts, frame, pose, ext[4:])
        occupancy = grid_ref.occupancy(counts, PARAMS["min_observations"])
        assert np.array_equal(np.fromfile(prefix + "_occupancy_%d.bin" % k, dtype=np.int8).reshape(H, W), occupancy)  # the readout never sees the plane
        costmap = np.fromfile(prefix + "_costmap_%d.bin" % k, dtype=np.uint8).reshape(H, W)
        assert np.array_equal(costmap, K.costmap_from_occupancy(tr.patched_readout(counts, want_plane, PARAMS["min_observations"]), table,
                                                                min_observations=PARAMS["min_observations"]))
        alone = K.costmap_from_occupancy(occupancy, table, min_observations=PARAMS["min_observations"])
        if k == BOX_FRAME:
            # the box: a transient on its cells, lethal in the costmap while the readout still calls them free
            on_box = want_plane.astype(bool) & box_cells
            assert on_box.sum() >= 3 and on_box.sum() == want_plane.sum() and len(want_rows) == 1
            assert (costmap[on_box] == 254).all() and (occupancy[on_box] >= 0).all() and (occupancy[on_box] <= 65).all() and (alone[on_box] < 253).any()
        if k == BOX_FRAME + 1:
            # the box has left: the plane is empty and the costmap is bit for bit what the counters alone give
            assert not want_plane.any() and len(want_rows) == 0 and np.array_equal(costmap, alone)
    assert at == len(rows_raw)
    assert np.array_equal(np.fromfile(prefix + "_counts.bin", dtype=np.uint16).reshape(H, W, 2), counts)
