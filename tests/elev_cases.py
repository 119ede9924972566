"""Inputs shared by the height columns' tests (tests/test_elev_host.py on the CPU, tests/test_gpu_elev.py on the GPU,
tests/test_elev_facade.py through the drop-in headers): seeded frames, poses, configurations and hand-made columns, so that the
stand-alone host program and the kernels are held to the restatement (tests/elev_ref.py) on the same data."""
import numpy as np

import elev_ref as er
import grid_cases as gc
from kinematic_icp_amd import synthetic as syn

IDENTITY = gc.IDENTITY
U64 = np.uint64
FULL = (1 << 64) - 1


def bits(*indices):
    return sum(1 << b for b in indices)


def pinned_8x6():
    """Seven returns seen from cell (0, 0) of an 8 x 6 layer of 1 m cells at the identity pose; slabs of 0.5 m from z = -1, so slab b is
    [-1 + b / 2, -1 + (b + 1) / 2).  Expected columns, cell by cell (every other column is zero):
        (7, 3): z = 0.0 -> bit 2, and z = 1.2 -> bit 4         (2, 5): z = 0.5 -> bit 3, twice
        (3, 1): z = -1.0 -> bit 0 (the lower border belongs)   (4, 1): z = 30.49 -> bit 62
    and one return at z = -1.01 (outside_column) and one at x = 8.5 (within reach, outside the grid).
    Classes at S = 1, H = 4: (7, 3) has ground 2 and bit 4 with 2 + 1 < 4 <= 2 + 4: BODY.  (4, 1) has ground 62 and its neighbour (3, 1)
    ground 0: 62 - 0 > 1: STEP, the higher cell of the edge; (3, 1) stays traversable.  (2, 5) is traversable."""
    cfg = er.make_config(1.0, 0.0, 0.0, 8, 6, -1.0, 0.5, 9.0)
    points = np.array([[7.5, 3.5, 0.0], [7.2, 3.1, 1.2], [2.5, 5.5, 0.5], [2.1, 5.9, 0.74], [3.5, 1.5, -1.0], [4.5, 1.5, 30.49], [3.5, 1.5, -1.01],
                       [8.5, 0.5, 0.0]])
    columns = {(7, 3): bits(2, 4), (2, 5): bits(3), (3, 1): bits(0), (4, 1): bits(62)}
    stats = (6, 0, 1, 1, 5, 4)
    classes = {(7, 3): 100, (2, 5): 0, (3, 1): 0, (4, 1): 100}
    return cfg, points, IDENTITY, np.array([0.5, 0.5, 0.0]), columns, stats, classes


def columns_array(cfg, columns):
    out = np.zeros((cfg["height"], cfg["width"]), dtype=U64)
    for (ix, iy), c in columns.items():
        out[iy, ix] = U64(c)
    return out


# a 16 x 16 layer of 0.25 m cells from (-2, -2), slabs of 0.125 m from z = -1 (all exact in binary); the sensor in cell (8, 8);
# reach = ceil(1.5 / 0.25) = 6 cells
CFG16 = er.make_config(0.25, -2.0, -2.0, 16, 16, -1.0, 0.125, 1.5)
SENSOR16 = np.array([0.1, 0.1, 0.0])
NAN, INF = float("nan"), float("inf")
# name -> (point, class, (ix, iy, slab) of a used one)
ONE_POINT = {
    "on_a_slab_border": ((0.3, 0.3, 0.25), er.USED, (9, 9, 10)),  # (0.25 + 1) / 0.125 is exactly 10: the border belongs to the upper slab
    "just_below_a_slab_border": ((0.3, 0.3, 0.25 - 2.0 ** -52), er.USED, (9, 9, 9)),  # 1.25 - 2^-52 is a double: the subtraction is exact
    "slab_0": ((0.3, 0.3, -1.0), er.USED, (9, 9, 0)),
    "slab_63": ((0.3, 0.3, np.nextafter(7.0, 0.0)), er.USED, (9, 9, 63)),
    "just_below_z_origin": ((0.3, 0.3, np.nextafter(-1.0, -2.0)), er.OUTSIDE_COLUMN, None),
    "at_the_column_top": ((0.3, 0.3, 7.0), er.OUTSIDE_COLUMN, None),  # z_origin + 64 slab
    "at_reach": ((1.6, 0.3, 0.0), er.USED, (14, 9, 8)),
    "beyond_reach": ((1.85, 0.3, 0.0), er.SKIPPED, None),
    "x_nan": ((NAN, 0.3, 0.0), er.SKIPPED, None), "y_nan": ((0.3, NAN, 0.0), er.SKIPPED, None), "z_nan": ((0.3, 0.3, NAN), er.SKIPPED, None),
    "x_inf": ((INF, 0.3, 0.0), er.SKIPPED, None), "y_inf": ((0.3, -INF, 0.0), er.SKIPPED, None), "z_inf": ((0.3, 0.3, INF), er.SKIPPED, None),
    "x_1e300": ((1.0e300, 0.3, 0.0), er.SKIPPED, None),
    "z_1e300": ((0.3, 0.3, 1.0e300), er.OUTSIDE_COLUMN, None),  # finite, so the cell counts before the column does
}
# the sensor in cell (13, 8) of the same layer: cell 16 is within reach and outside the grid
SENSOR16_EAST = np.array([1.35, 0.1, 0.0])
INSIDE_REACH_OUTSIDE_GRID = np.array([[2.1, 0.1, 0.0]])


def contended_three(n=4096, seed=5):
    """n points spread over three (cell, slab) pairs of CFG16"""
    rng = np.random.default_rng(seed)
    corners = np.array([[1.0, 0.5, 0.0], [-0.75, 1.0, 0.5], [0.25, -1.25, -0.5]])  # lower corners of three cells and of three slabs
    return corners[rng.integers(0, 3, n)] + rng.uniform(0.01, 0.24, (n, 3)) * np.array([1.0, 1.0, 0.5])


def contended_one_cell(n=4096, seed=6):
    """n points in ONE cell of CFG16 over all 64 slabs (every slab is drawn: n is 64 times 64)"""
    rng = np.random.default_rng(seed)
    slab = rng.permutation(np.arange(n) % 64)
    z = -1.0 + 0.125 * slab + rng.uniform(0.0, 0.12, n)
    return np.concatenate([np.array([0.5, 0.5]) + rng.uniform(0.01, 0.24, (n, 2)), z[:, None]], axis=1)


def tilted_frame(n=3000, seed=7):
    """a pose with roll and pitch, so that wz depends on x and y: (points, pose, sensor)"""
    rng = np.random.default_rng(seed)
    pose = gc.tilted_pose(0.2, -0.1, 0.7, np.deg2rad(9.0), np.deg2rad(-6.0), z=0.3)
    pts = np.concatenate([rng.uniform(-1.9, 1.9, (n, 2)), rng.uniform(-1.2, 1.0, (n, 1))], axis=1)
    return np.ascontiguousarray(pts), pose, SENSOR16


DRIVE_EXT = np.concatenate([[0, 0, np.sin(0.05), np.cos(0.05)], [0.3, 0.0, 0.9]])  # lidar_to_base of tests/test_grid_facade.py's drive


def drive_scene():
    """the scene with boxes and the 12 x 512 beams of tests/test_grid_facade.py's drive"""
    rng = np.random.Generator(np.random.PCG64(77))
    scene = syn.make_scene(rng, half=16.0, height=4.0, n_boxes=6, box_xy=(2.0, 5.0), box_z=(1.5, 3.5), keep_clear=3.0)
    return rng, scene, syn.beam_directions(12, 512, (-20.0, 8.0))


def random_drive():
    """Six frames of that scene in the base frame, the robot rolling and pitching by a few degrees; the last pose near the border, so
    that the window is clipped; a few non-finite coordinates included.  The layer: 0.1 m cells from (-14, -14) to (16, 16), so the
    scene's walls at -16 lie outside the grid; slabs of 0.0625 m from 1 m below the floor, so the column ends at 3 m and the ceiling at
    4 m lies outside it; reach 120 cells: the far walls are skipped."""
    cfg = er.make_config(0.1, -14.0, -14.0, 300, 300, -1.0, 0.0625, 12.0)
    rng, scene, dirs = drive_scene()
    places = [(0.0, 0.0), (0.4, 0.1), (0.9, 0.3), (1.5, 0.2), (-5.0, 4.0), (12.0, -13.5)]
    frames = []
    for k, (x, y) in enumerate(places):
        pose = gc.tilted_pose(x, y, 0.1 + 0.4 * k, np.deg2rad(rng.uniform(-4, 4)), np.deg2rad(rng.uniform(-4, 4)), z=rng.uniform(-0.05, 0.05))
        world_from_lidar = syn.pose_mul(pose, DRIVE_EXT)
        R = syn.quat_to_matrix(world_from_lidar[:4])
        t = scene.raycast(world_from_lidar[4:], dirs @ R.T) + rng.normal(0, 0.01, len(dirs))
        pts = syn.pose_act(DRIVE_EXT, dirs * t[:, None])  # lidar frame -> base frame
        pts[rng.integers(0, len(pts), 3), rng.integers(0, 3, 3)] = [np.nan, np.inf, -np.inf]
        frames.append((np.ascontiguousarray(pts), pose, DRIVE_EXT[4:].copy()))
    return cfg, frames


def reference_run(cfg, frames):
    """-> (columns after every frame, stats of every frame) by the restatement"""
    columns = np.zeros((cfg["height"], cfg["width"]), dtype=U64)
    after, stats = [], []
    for pts, pose, sensor in frames:
        stats.append(er.integrate(cfg, columns, pts, pose, sensor))
        after.append(columns.copy())
    return after, stats


def write_frames(path, cfg, frames, params):
    """the input file of tests/cpp/elev_host_test.cpp; params: the (S, H) pairs it classifies the final columns with"""
    with open(path, "wb") as f:
        np.array([cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_origin"], cfg["slab"], cfg["max_ray"], len(frames), len(params)],
                 dtype=np.float64).tofile(f)
        np.array(params, dtype=np.float64).reshape(-1, 2).tofile(f)
        for pts, pose, sensor in frames:
            np.concatenate([np.asarray(pose, dtype=np.float64), np.asarray(sensor, dtype=np.float64), [float(len(pts))]]).tofile(f)
            np.ascontiguousarray(pts, dtype=np.float64).tofile(f)


# ---- classification: a 70 x 45 layer (no multiple of the 16-cell tile), hand-made columns -------------------------------------------
W70, H45 = 70, 45
# (S, H) pairs: the least, a usual one, the largest step with the least robot over it, the tallest robot with and without a step
PARAMS = [(0, 1), (2, 8), (62, 63), (0, 64), (5, 64)]


def handmade_columns():
    """the columns the shifts by 64 and the tile borders can get wrong (tiles are 16 x 16 from the rectangle's corner)"""
    c = np.zeros((H45, W70), dtype=object)
    c[8, 2] = bits(63)                         # only the top bit: g + S + 1 >= 64 for every S
    c[8, 5] = bits(60, 63)                     # a ground at 60: with H = 64, g + H passes 63
    c[8, 8] = bits(60, 61)
    c[8, 11] = FULL                            # a full column
    c[8, 14] = bits(0, 63)                     # S = 62, H = 63: bit 63 is the one bit in (0 + 62, 0 + 63]
    c[8, 17] = bits(0, 62)                     # ... and bit 62 is not
    c[8, 20] = bits(1, 63)                     # g + S + 1 = 64 at S = 62
    c[5, 2], c[5, 3] = bits(0), bits(1)        # S = 0: one slab is a step
    for x, y in ((15, 20), (31, 20), (47, 20), (63, 20)):  # a STEP pair across every vertical tile border, the higher cell on either side
        c[y, x], c[y, x + 1] = bits(3), bits(30)
        c[y + 2, x], c[y + 2, x + 1] = bits(30), bits(3)
    for x, y in ((20, 15), (20, 31), (40, 15), (40, 31)):  # ... across every horizontal one, and diagonally across a tile corner
        c[y, x], c[y + 1, x] = bits(3), bits(30)
        c[y, x + 3], c[y + 1, x + 3] = bits(30), bits(3)
    c[15, 31], c[16, 32] = bits(2), bits(40)
    c[16, 47], c[15, 48] = bits(2), bits(40)
    for x, y, nx, ny in ((0, 0, 1, 1), (W70 - 1, 0, W70 - 2, 0), (0, H45 - 1, 0, H45 - 2), (W70 - 1, H45 - 1, W70 - 2, H45 - 2)):  # each grid corner:
        c[y, x], c[ny, nx] = bits(20), bits(1)  # the corner is the higher cell; its other neighbours lie outside the grid or are unknown
    c[30, 60] = bits(9)                        # known, every neighbour unknown
    c[36, 0], c[36, 1] = bits(1), bits(20)     # the higher cell beside the grid's edge
    return c.astype(U64)


def random_columns(kind, seed=11):
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << 63, (H45, W70), dtype=U64) << U64(1) | rng.integers(0, 2, (H45, W70), dtype=U64)
    if kind == "dense":
        return words
    if kind == "sparse":  # few bits per column, many unknown cells: grounds and steps of every size
        few = (U64(1) << rng.integers(0, 64, (H45, W70), dtype=U64)) | (U64(1) << rng.integers(0, 64, (H45, W70), dtype=U64))
        return few * (rng.random((H45, W70)) < 0.6).astype(U64)
    assert kind == "zero"
    return np.zeros((H45, W70), dtype=U64)


# the full layer, a 1 x 1 rectangle at each corner, and rectangles whose corners and tiles straddle the full layer's tile borders
RECTS = [None, (0, 0, 1, 1), (W70 - 1, 0, 1, 1), (0, H45 - 1, 1, 1), (W70 - 1, H45 - 1, 1, 1), (15, 15, 2, 2), (14, 19, 35, 5), (31, 0, 17, 45), (1, 1, 68, 43),
         (47, 14, 23, 19)]
