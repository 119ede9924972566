"""The scenes of the transient tests (tests/test_transient_host.py, tests/test_gpu_transients.py): per scene a grid's configuration -
K.OccupancyGrid's arguments - its counters, one frame of points in the base frame with its pose and sensor, and the detection's four
parameters.  Points are the centres of the cells they are meant for, so no rounding decides where one falls."""
import math

import numpy as np

import grid_ref

IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
FREE, UNKNOWN, WALL, BUSY = (0, 20), (0, 0), (20, 0), (6, 4)  # (hits, misses): readouts 0, -1, 100 and 60


def grid_args(width, height, max_ray=12.0, cell=0.1, origin=(-1.0, -2.0)):
    return (cell, origin[0], origin[1], int(width), int(height), 0.0, 1.0, float(max_ray))


def free_counts(width, height, pair=FREE):
    counts = np.zeros((height, width, 2), dtype=np.uint16)
    counts[...] = pair
    return counts


def pose_of(yaw, tx, ty):
    return np.array([0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2), tx, ty, 0.0])


def points_at(args, cells, pose=IDENTITY, z=0.5):
    """the centres of `cells` = [(x, y, n), ...] (n returns each; cells outside the grid are fine) as points in the base frame of `pose`
    (a yaw and a translation)"""
    cell, ox, oy = args[0], args[1], args[2]
    xs = np.repeat([c[0] for c in cells], [c[2] for c in cells]).astype(np.float64)
    ys = np.repeat([c[1] for c in cells], [c[2] for c in cells]).astype(np.float64)
    wx, wy = ox + (xs + 0.5) * cell - pose[4], oy + (ys + 0.5) * cell - pose[5]
    yaw = 2.0 * math.atan2(pose[2], pose[3])
    c, s = math.cos(yaw), math.sin(yaw)
    return np.ascontiguousarray(np.stack([c * wx + s * wy, -s * wx + c * wy, np.full(len(xs), z)], axis=1))


def sensor_at(args, x, y, pose=IDENTITY):
    """the sensor's position in the base frame that puts it into the middle of cell (x, y)"""
    return points_at(args, [(x, y, 1)], pose, 0.2)[0]


def scene(args, counts, cells, sensor_cell=(3, 3), pose=IDENTITY, extra=None, **params):
    pts = points_at(args, cells, pose)
    if extra is not None:
        pts = np.ascontiguousarray(np.concatenate([pts, np.asarray(extra, dtype=np.float64).reshape(-1, 3)]))
    p = dict(min_observations=1, free_max=65, min_points=1, min_size=1)
    p.update(params)
    return dict(args=args, cfg=grid_ref.make_config(*args), counts=counts, points=pts, pose=np.asarray(pose, dtype=np.float64),
                sensor=sensor_at(args, sensor_cell[0], sensor_cell[1], pose), params=p)


def pinned_8x6():
    """An 8 x 6 grid of 1 m cells from (0, 0), the sensor in cell (0, 0), min_points 2, free_max 65, min_size 2; row y = 5 on top.  Left the
    counters - `.` free (readout 0), `u` unknown, `S` occupied (100), `b` busy (60: still at or below 65) - right the returns n(c):
        y 5   . . . . . . . .          . . . . . . . 1
        y 4   . . u . . . S .          . . 9 . 2 . 5 .
        y 3   . . . . . . . .          . . . . . . . .
        y 2   . . . . . b . .          . . 3 . . 4 2 .
        y 1   . . . . . . . .          . 2 . 2 . . . .
        y 0   . . . . . . . .          . . . . . . . .
    and three used points that end in cell (9, 2), outside the grid, and one above the band.  Transient cells: A = 9, 11, 18 (joined
    through corners; label 9), B = 21, 22 (label 21) and C = 36 alone, which min_size drops from the rows and the plane but not from
    the labels; cell 47 has one return of the two it needs.
    -> (the scene, labels, rows, plane, stats)"""
    args = (1.0, 0.0, 0.0, 8, 6, 0.0, 1.0, 20.0)
    counts = free_counts(8, 6)
    counts[4, 2], counts[4, 6], counts[2, 5] = UNKNOWN, WALL, BUSY
    cells = [(1, 1, 2), (2, 2, 3), (3, 1, 2), (5, 2, 4), (6, 2, 2), (2, 4, 9), (6, 4, 5), (7, 5, 1), (4, 4, 2), (9, 2, 3)]
    s = scene(args, counts, cells, sensor_cell=(0, 0), extra=[[3.5, 3.5, 1.5]], min_points=2, min_size=2)
    labels = np.full(48, 0xFFFFFFFF, dtype=np.uint32)
    labels[[9, 11, 18]], labels[[21, 22]], labels[36] = 9, 21, 36
    rows = np.array([[9, 3, 2 + 3 + 2, 2 * 1 + 3 * 2 + 2 * 3, 2 * 1 + 3 * 2 + 2 * 1, 1, 3, 1, 2, ((1 + 1) << 32) + 9],
                     [21, 2, 4 + 2, 4 * 5 + 2 * 6, 4 * 2 + 2 * 2, 5, 6, 2, 2, ((25 + 4) << 32) + 21]], dtype=np.uint64)
    plane = np.zeros(48, dtype=np.uint8)
    plane[[9, 11, 18, 21, 22]] = 1
    return s, labels.reshape(6, 8), rows, plane.reshape(6, 8), (33, 30, 9, 6)


def random_scene(width, height, seed, n=None, max_ray=40.0):
    """random counters - a fifth unknown, the rest anything from free to occupied - and a frame of n returns, half of them scattered over
    a rectangle somewhat larger than the grid and half in clusters, seen from the grid's middle at a yawed pose"""
    rng = np.random.default_rng(seed)
    args = grid_args(width, height, max_ray)
    counts = np.stack([rng.integers(0, 30, (height, width)), rng.integers(0, 60, (height, width))], axis=2).astype(np.uint16)
    counts[rng.random((height, width)) < 0.2] = 0
    n = width * height // 3 + 5 if n is None else n
    xs, ys = rng.integers(-3, width + 3, n), rng.integers(-3, height + 3, n)
    k = n // 2
    centres = rng.integers(0, [width, height], (max(k // 40, 1), 2))
    pick = rng.integers(0, len(centres), k)
    xs[:k], ys[:k] = centres[pick, 0] + rng.integers(-2, 3, k), centres[pick, 1] + rng.integers(-2, 3, k)
    cells = [(int(x), int(y), 1) for x, y in zip(xs, ys)]
    return scene(args, counts, cells, sensor_cell=(width // 2, height // 2), pose=pose_of(0.3 + 0.1 * seed, 0.4, -0.3), min_points=1 + seed % 2, min_size=1 + seed % 3)


def switch_scene(width=90, height=70, seed=7):
    """a mostly free grid with a sprinkle of occupied cells and two unknown patches, and a frame that drops a few boxes of returns and
    some lone ones into it: a costmap with room to plan in, which the transients change"""
    rng = np.random.default_rng(seed)
    args = grid_args(width, height)
    counts = free_counts(width, height)
    for x, y in rng.integers(0, [width, height], (width * height // 100, 2)):
        counts[y, x] = WALL
    counts[10:22, 60:75], counts[50:58, 5:30] = UNKNOWN, UNKNOWN
    cells = [(int(cx) + dx, int(cy) + dy, 2) for cx, cy in rng.integers(4, [width - 4, height - 4], (8, 2)) for dx in range(3) for dy in range(3)]
    cells += [(int(x), int(y), 1) for x, y in rng.integers(0, [width, height], (40, 2))]
    return scene(args, counts, cells, sensor_cell=(width // 2, height // 2), pose=pose_of(-0.4, 0.2, 0.1), min_size=2)


def cases():
    """name -> scene: the issue's list but for the large frames (random_scene(260, 200, seed, 20000), which the GPU test makes itself)"""
    out = {"pinned_8x6": pinned_8x6()[0]}
    for k, (w, h) in enumerate([(31, 31), (32, 32), (33, 33), (63, 65), (64, 64), (65, 63), (1, 1), (1, 70), (70, 1)]):
        out["random_%dx%d" % (w, h)] = random_scene(w, h, 20 + k)
    a = grid_args(64, 64)
    out["corner_pair_31_31_32_32"] = scene(a, free_counts(64, 64), [(31, 31, 2), (32, 32, 1)])
    out["corner_pair_32_31_31_32"] = scene(a, free_counts(64, 64), [(32, 31, 1), (31, 32, 3)])
    a = grid_args(70, 70)
    out["along_a_tile_border"] = scene(a, free_counts(70, 70), [(x, y, 1 + x % 3) for x in range(5, 61) for y in (31, 32)] + [(x, y, 1) for y in range(40, 66) for x in (31, 32)])
    out["two_blobs_touch_at_a_corner"] = scene(a, free_counts(70, 70), [(x, y, 2) for x in (10, 11) for y in (10, 11)] + [(x, y, 1) for x in (12, 13) for y in (12, 13)],
                                               sensor_cell=(40, 5))
    out["two_apart"] = scene(a, free_counts(70, 70), [(10, 10, 1), (12, 10, 1), (10, 12, 1)])
    out["min_points_boundary"] = scene(a, free_counts(70, 70), [(20, 20, 2), (40, 40, 3)], min_points=3)
    counts = free_counts(70, 70)
    counts[20, 20], counts[40, 40], counts[50, 50] = (65, 35), (66, 34), (0, 0)
    out["free_max_boundary"] = scene(a, counts, [(20, 20, 1), (40, 40, 1)])
    out["unknown_under_many_returns"] = scene(a, counts, [(50, 50, 50), (51, 50, 1)])
    counts = free_counts(70, 70)
    counts[20, 20] = (0, 3)
    out["min_observations_turns_unknown"] = scene(a, counts, [(20, 20, 4), (40, 40, 4)], min_observations=5)
    # max_ray 4 m: a reach of 40 cells around the sensor's cell (5, 35); cell (45, 35) lies at 40, (47, 35) at 42
    near = grid_args(70, 70, max_ray=4.0)
    inf, nan = float("inf"), float("nan")
    out["skipped_returns"] = scene(near, free_counts(70, 70), [(6, 36, 2), (45, 35, 1), (47, 35, 3), (-2, 30, 2), (80, 36, 3), (5, 76, 1)], sensor_cell=(5, 35),
                                   extra=[[0.5, 0.5, 1.0], [0.5, 0.5, -0.1], [nan, 0.0, 0.5], [0.0, inf, 0.5], [0.0, 0.0, nan], [1e300, 0.0, 0.5]])
    out["sensor_outside_the_grid"] = scene(a, free_counts(70, 70), [(2, 30, 2), (3, 31, 1), (60, 60, 1)], sensor_cell=(-20, 30))
    out["sensor_far_outside"] = scene(near, free_counts(70, 70), [(2, 30, 2)], sensor_cell=(-60, 30))
    out["5000_returns_in_one_cell"] = scene(a, free_counts(70, 70), [(33, 34, 5000), (34, 34, 7)])
    out["no_points"] = scene(a, free_counts(70, 70), [])
    out["no_transient"] = scene(a, free_counts(70, 70, WALL), [(10, 10, 3), (11, 10, 1)])
    # the four edge neighbours of the sensor's cell (32, 32), joined through their corners, all at distance 1: the least index wins word 9
    out["nearest_ties"] = scene(a, free_counts(70, 70), [(33, 32, 1), (32, 33, 2), (31, 32, 1), (32, 31, 1), (50, 30, 1), (50, 34, 1), (51, 32, 1)], sensor_cell=(32, 32))
    out["yawed_pose"] = scene(a, free_counts(70, 70), [(10 + k, 20 + k // 2, 1 + k % 2) for k in range(30)], sensor_cell=(5, 5), pose=pose_of(2.1, 1.5, -0.7))
    return out
