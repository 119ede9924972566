"""Following through the drop-in C++ headers (tests/cpp/scroll_facade_test.cpp): the drive of tests/test_transient_facade.py, without
its box and two frames longer, through KinematicICP with a grid and a height layer of 128 x 128 cells of 0.1 m - small enough that the
robot leaves the band of margin 60 and step 4 several times, large enough to hold walls that return.  After every frame the counters
and the columns must equal the restatement: the follow rule at the returned pose (tests/scroll_ref.py), the shift, then the frame
integrated at the reported origin (tests/grid_ref.py, tests/elev_ref.py); poses and clouds must be bit-equal with and without
following."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kinematic_icp_amd import synthetic as syn
import elev_cases as ec
import elev_ref
import grid_ref
import scroll_ref as sr

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "scroll_facade_test")
GRID = (0.1, -6.4, -6.4, 128, 128, 0.1, 1.5, 12.0)
MARGIN, STEP, Z_ORIGIN, SLAB = 60, 4, -1.0, 0.0625
N_FRAMES = 8


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "scroll_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_scroll_facade_compiles_and_links():
    assert os.path.exists(build_binary())


def drive():
    """tests/test_grid_facade.py's drive (deskew on), N_FRAMES frames -> (lidar_to_base, true poses in the first pose's frame, frames,
    stamps, odometry deltas)"""
    rng, scene, dirs = ec.drive_scene()
    ext = ec.DRIVE_EXT
    poses, frames, stamps, deltas = [syn.planar_pose(0.0, 0.0, 0.1)], [], [], []
    for k in range(N_FRAMES):
        delta_true = syn.planar_pose(0.25, 0.0, np.deg2rad(2.0 + k))
        poses.append(syn.pose_mul(poses[-1], delta_true))
        world_from_lidar = syn.pose_mul(poses[-1], ext)
        R = syn.quat_to_matrix(world_from_lidar[:4])
        t = scene.raycast(world_from_lidar[4:], dirs @ R.T) + rng.normal(0, 0.01, len(dirs))
        frames.append(dirs * t[:, None])
        stamps.append(np.linspace(0.0, 1.0, len(dirs)))
        deltas.append(syn.pose_mul(delta_true, syn.planar_pose(0.01 * (-1) ** k, 0.0, np.deg2rad(0.15))))
    start = syn.pose_inverse(poses[0])
    return ext, [syn.pose_mul(start, p) for p in poses[1:]], frames, stamps, deltas


def write_drive(path):
    ext, _, frames, stamps, deltas = drive()
    with open(path, "wb") as fh:
        np.array([len(frames), 0.5, 30.0, 1.0]).tofile(fh)
        ext.tofile(fh)
        for fr, st, dl in zip(frames, stamps, deltas):
            np.array([float(len(fr))]).tofile(fh)
            np.ascontiguousarray(fr).tofile(fh), st.tofile(fh), dl.tofile(fh)
    return ext


def follow_all(positions):
    """the follow rule along a list of (x, y) with the chosen numbers -> the shifts (dx, dy) per position"""
    ox, oy, out = GRID[1], GRID[2], []
    for x, y in positions:
        dx, dy = sr.follow(x, y, ox, oy, GRID[0], GRID[3], GRID[4], MARGIN, STEP)
        ox, oy = sr.origin(ox, dx, GRID[0]), sr.origin(oy, dy, GRID[0])
        out.append((dx, dy))
    return out


def test_the_chosen_numbers_scroll_at_least_twice_along_x():
    """on the CPU, by the restatement alone: along the drive's true poses the band of MARGIN and STEP is left at least twice towards
    +x - and even a metre of registration error per frame could not make it never"""
    _, poses, _, _, _ = drive()
    shifts = follow_all([(p[4], p[5]) for p in poses])
    print("true positions", [(round(p[4], 2), round(p[5], 2)) for p in poses], "shifts", shifts)
    assert sum(1 for dx, _ in shifts if dx > 0) >= 3 and all(dx >= 0 and dx % STEP == 0 and dy % STEP == 0 for dx, dy in shifts)
    assert shifts[0] == (0, 0)  # the first frame stays inside the band: following begins from a grid that has seen a frame
    assert 2 * MARGIN + STEP <= min(GRID[3], GRID[4])


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
def test_following_through_the_pipeline(tmp_path):
    f, g, prefix = tmp_path / "pipe.bin", tmp_path / "grid.bin", str(tmp_path / "out")
    ext = write_drive(f)
    np.array(list(GRID) + [MARGIN, STEP, Z_ORIGIN, SLAB], dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    for line in ["refused_without_grid 1", "off_by_default 1", "refused_bad_pair 1", "enabled 1", "copy_carries_the_setting 1", "moved_carries_the_setting 1",
                 "plain_never_scrolls 1", "disabled 1", "new_handles_start_off 1"]:
        assert line in out, (line, out)

    # poses and returned clouds: bit-equal without and with following
    assert open(prefix + "_off.bin", "rb").read() == open(prefix + "_on.bin", "rb").read()
    run = read_run(prefix + "_on.bin", N_FRAMES)
    H, W = GRID[4], GRID[3]
    scrolls = np.fromfile(prefix + "_scrolls.bin", dtype=np.int32).reshape(N_FRAMES, 4)
    origins = np.fromfile(prefix + "_origins.bin", dtype=np.float64).reshape(N_FRAMES, 4)
    all_counts = np.fromfile(prefix + "_counts.bin", dtype=np.uint16).reshape(N_FRAMES, H, W, 2)
    all_columns = np.fromfile(prefix + "_columns.bin", dtype=np.uint64).reshape(N_FRAMES, H, W)
    print("LastGridScroll per frame", scrolls[:, :2].tolist())
    assert int((scrolls[:, 0] > 0).sum()) >= 2  # a drive that never scrolls cannot pass
    assert np.array_equal(scrolls[:, :2], scrolls[:, 2:])  # the same rule, the same origin: the layer scrolls with the grid
    assert scrolls.tolist() == [list(d) * 2 for d in follow_all([(pose[4], pose[5]) for pose, _, _ in run])]

    gcfg = grid_ref.make_config(*GRID)
    ecfg = elev_ref.make_config(GRID[0], GRID[1], GRID[2], W, H, Z_ORIGIN, SLAB, GRID[7])
    counts, columns = np.zeros((H, W, 2), dtype=np.uint16), np.zeros((H, W), dtype=np.uint64)
    for k, (pose, frame, _) in enumerate(run):
        dx, dy = sr.follow(pose[4], pose[5], gcfg["origin_x"], gcfg["origin_y"], GRID[0], W, H, MARGIN, STEP)
        counts, columns = sr.shift(counts, dx, dy), sr.shift(columns, dx, dy)
        for cfg in (gcfg, ecfg):
            cfg["origin_x"], cfg["origin_y"] = sr.origin(cfg["origin_x"], dx, GRID[0]), sr.origin(cfg["origin_y"], dy, GRID[0])
        assert origins[k].tolist() == [gcfg["origin_x"], gcfg["origin_y"], ecfg["origin_x"], ecfg["origin_y"]], k
        grid_ref.integrate(gcfg, counts, frame, pose, ext[4:])
        elev_ref.integrate(ecfg, columns, frame, pose, ext[4:])
        assert np.array_equal(all_counts[k], counts), (k, np.argwhere(all_counts[k] != counts)[:4])
        assert np.array_equal(all_columns[k], columns), (k, np.argwhere(all_columns[k] != columns)[:4])
        # the robot's cell lies inside the band after every frame
        assert MARGIN <= sr.cell_of(pose[4], gcfg["origin_x"], GRID[0]) < W - MARGIN and MARGIN <= sr.cell_of(pose[5], gcfg["origin_y"], GRID[0]) < H - MARGIN
    assert counts[..., 0].any() and counts[..., 1].any() and columns.any()  # hits, misses and heights: the drive drew something
