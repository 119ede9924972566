"""Inputs shared by the tests of the height columns' carve (tests/test_elev_carve_host.py on the CPU, tests/test_gpu_elev_carve.py on
the GPU, tests/test_elev_carve_facade.py through the drop-in headers): hand-made rays on hand-set columns, one case per regime the
arithmetic or the kernels can get wrong, each with a predicate that says the case does enter its regime (`enters`, evaluated on the
CPU against tests/elev_carve_ref.py), and the passer-by drive.

A case: cfg, start (the columns before the first frame), frames - (points, pose, sensor, (G, W, keep_ground)) each - and enters, a
function of the case and of the restatement's nine words per frame."""
import functools

import numpy as np

import elev_carve_ref as ecr
import elev_cases as ec
import elev_ref as er
import grid_cases as gc
from kinematic_icp_amd import synthetic as syn

U64 = np.uint64
CFG16 = ec.CFG16  # 16 x 16 cells of 0.25 m from (-2, -2), slabs of 0.125 m from z = -1, reach 6
NAN = float("nan")


def at(ix, iy, slab, cfg=CFG16):
    """the middle of cell (ix, iy) and of slab `slab` (any integer: the column is slabs 0 .. 63), a point in the world"""
    return [cfg["origin_x"] + (ix + 0.5) * cfg["cell"], cfg["origin_y"] + (iy + 0.5) * cfg["cell"], cfg["z_origin"] + (slab + 0.5) * cfg["slab"]]


def pts(*triples, cfg=CFG16):
    return np.array([at(*t, cfg=cfg) for t in triples], dtype=np.float64).reshape(-1, 3)


def full(cfg=CFG16):
    return np.full((cfg["height"], cfg["width"]), ec.FULL, dtype=U64)


def zeros(cfg=CFG16):
    return np.zeros((cfg["height"], cfg["width"]), dtype=U64)


def dense(cfg=CFG16, seed=21):
    """random columns, about half the bits set"""
    rng = np.random.default_rng(seed)
    shape = (cfg["height"], cfg["width"])
    return rng.integers(0, 1 << 63, shape, dtype=U64) << U64(1) | rng.integers(0, 2, shape, dtype=U64)


def frame(points, sensor, params, pose=ec.IDENTITY):
    return (np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(pose, dtype=np.float64), np.asarray(sensor, dtype=np.float64), tuple(params))


def spans(case, k=0):
    points, pose, sensor, (G, W, _) = case["frames"][k]
    return ecr.steps(case["cfg"], points, pose, sensor, G, W, spans=True)


def lengths(case, k=0):
    """(m, d) of every distinct ray of frame k"""
    points, pose, sensor, _ = case["frames"][k]
    _, tri, ss = ecr.triples(case["cfg"], points, pose, sensor)
    return [(max(abs(a), abs(b)), c - ss) for a, b, c in tri]


def pinned_8x6(keep_ground):
    """Two returns seen from cell (0, 0) of elev_cases.pinned_8x6()'s layer (1 m cells, slabs of 0.5 m from z = -1) at the identity pose,
    the sensor at z = 0: ss = 2.  G = 1, W = 0.  Written out by hand:
      the return at (4.5, 0.5, 2.0): cell (4, 0), es = 6, m = 4, d = 4, u(j) = 2 + (4 j + 4) / 8 = 2 3 3 4 4 5 5 6 for j = 0 .. 7; steps
        k = 0: u(0) .. u(1) = bits 2 .. 3 of cell (0, 0);  k = 1: u(1) .. u(3) = bits 3 .. 4 of (1, 0);  k = 2: u(3) .. u(5) = bits 4 .. 5 of
        (2, 0);  k = 3 falls to the margin: (3, 0) is left alone, and (4, 0) is the endpoint
      the return at (0.5, 3.5, -1.0): cell (0, 3), es = 0, m = 3, d = -2, u(j) = 2 - (2 j + 3) / 6 = 2 2 1 1 for j = 0 .. 3; steps
        k = 0: bit 2 of (0, 0);  k = 1: u(1) .. u(3) = bits 1 .. 2 of (0, 1);  k = 2 falls to the margin
    Cells (0 .. 4, 0) start as 0xFF, (0, 1) as bits 1 and 2, everything else empty.  (0, 1) keeps its ground, bit 1, with keep_ground and
    is emptied without.  The mark sets bit 6 of (4, 0), which is set, and bit 0 of (0, 3): one new bit in one new cell.
    -> (cfg, start, points, pose, sensor, (G, W, keep_ground), expected columns {(ix, iy): column}, the nine words)"""
    cfg = ec.pinned_8x6()[0]
    start = {(x, 0): 0xFF for x in range(5)}
    start[(0, 1)] = ec.bits(1, 2)
    points = np.array([[4.5, 0.5, 2.0], [0.5, 3.5, -1.0]])
    want = {(0, 0): 0xF3, (1, 0): 0xE7, (2, 0): 0xCF, (3, 0): 0xFF, (4, 0): 0xFF, (0, 3): 0x01}
    if keep_ground:
        want[(0, 1)] = ec.bits(1)
    stats = (2, 0, 0, 0, 1, 1, 2, 7, 0) if keep_ground else (2, 0, 0, 0, 1, 1, 2, 8, 1)
    return cfg, ec.columns_array(cfg, start), points, ec.IDENTITY, np.array([0.5, 0.5, 0.0]), (1, 0, keep_ground), want, stats


S8 = at(8, 8, 8)  # the sensor of most cases: cell (8, 8), slab 8
EAST = pts((14, 8, 63), (14, 9, 63), (13, 14, 40), (3, 2, 63))  # rays that climb to the column's top


def _case(frames, start, enters, cfg=CFG16):
    return dict(cfg=cfg, start=start, frames=frames, enters=enters)


# ---- masks ------------------------------------------------------------------------------------------------------------------------
def mask_reaching_bit_63():
    """a full column under a mask whose hi is exactly 63 (hi + 1 == 64) - and, with W = 5, under masks that end below and above it"""
    def enters(case, stats):
        lo, hi = spans(case)
        return (hi == 63).any() and (hi < 63).any() and stats[0][7] > 0
    return _case([frame(EAST, S8, (0, 5, 0))], full(), enters)


def mask_hi_64_and_above():
    def enters(case, stats):
        lo, hi = spans(case)
        return ((hi >= 64) & (lo <= 63) & (lo >= 0)).any() and (hi == 64).any() and (lo > 63).any()  # cut at the top, and wholly above
    return _case([frame(pts((14, 8, 75), (2, 8, 64), (8, 14, 200), (9, 9, 32767), (9, 8, 120)), S8, (0, 0, 0))], full(), enters)  # (9, 8, 120): slabs 8 .. 64


def mask_lo_below_0():
    def enters(case, stats):
        lo, hi = spans(case)
        return ((lo < 0) & (hi >= 0)).any() and (hi < 0).any() and (lo == -1).any()  # cut at the bottom, and wholly below
    return _case([frame(pts((14, 8, -20), (9, 8, -9), (8, 14, -200), (9, 9, -32768)), S8, (0, 0, 0)),  # (9, 8, -9): slabs -1 .. 8
                  frame(pts((14, 8, -20), (2, 8, -1)), S8, (0, 1, 1))], full(), enters)


def spans_wholly_outside():
    """a sensor above the column looking up and one below it looking down: every span lies outside, nothing is cleared"""
    def enters(case, stats):
        (lo0, hi0), (lo1, hi1) = spans(case, 0), spans(case, 1)
        return len(lo0) > 0 and (lo0 > 63).all() and len(lo1) > 0 and (hi1 < 0).all() and stats[0][6:] == (3, 0, 0) and stats[1][6:] == (3, 0, 0)
    up, down = pts((14, 8, 90), (2, 3, 64 + 3), (8, 13, 300)), pts((14, 8, -30), (2, 3, -4), (8, 13, -300))
    return _case([frame(up, at(8, 8, 66), (0, 2, 0)), frame(down, at(8, 8, -3), (0, 2, 0))], full(), enters)


def sensor_above_and_below_the_column():
    """ss above 63 looking down into the column, ss below 0 looking up into it"""
    def enters(case, stats):
        (lo0, hi0), (lo1, hi1) = spans(case, 0), spans(case, 1)
        return ecr.sensor(case["cfg"], *case["frames"][0][1:3])[2] == 70 and ecr.sensor(case["cfg"], *case["frames"][1][1:3])[2] == -7 and \
            (lo0 > 63).any() and ((hi0 >= 64) & (lo0 <= 63)).any() and (hi0 <= 63).any() and (hi1 < 0).any() and ((lo1 < 0) & (hi1 >= 0)).any() and (lo1 >= 0).any() and \
            stats[0][7] > 0 and stats[1][7] > 0
    targets = pts((14, 8, 5), (13, 13, 30), (2, 8, 0), (8, 2, 63), (3, 3, 9))
    return _case([frame(targets, at(8, 8, 70), (0, 0, 0)), frame(targets, at(8, 8, -7), (0, 1, 1))], dense(), enters)


def widen(W):
    def build():
        def enters(case, stats):
            lo, hi = spans(case)
            return ((hi - lo) >= 2 * W).all() and ((hi - lo) == 2 * W).any() and stats[0][7] > 0 and (W < 64 or ((lo < 0) & (hi > 63)).all())
        return _case([frame(pts((14, 8, 8), (13, 13, 30), (2, 8, 0), (8, 2, 63), (3, 3, 9), (9, 8, 20)), S8, (0, W, 0))], dense(), enters)
    return build


# ---- ray shapes ---------------------------------------------------------------------------------------------------------------------
def level_rays():
    """d = 0: every step's span is the sensor's slab"""
    def enters(case, stats):
        lo, hi = spans(case)
        return all(d == 0 for _, d in lengths(case)) and (lo == 8).all() and (hi == 8).all() and stats[0][7] > 0
    return _case([frame(pts((14, 8, 8), (2, 3, 8), (8, 14, 8), (11, 12, 8)), S8, (0, 0, 0))], full(), enters)


def steep_rays():
    """|d| > m, up and down, m = 1 among them: a step spans many slabs"""
    def enters(case, stats):
        ms = lengths(case)
        lo, hi = spans(case)
        return all(abs(d) > m for m, d in ms) and any(m == 1 for m, _ in ms) and (hi - lo).max() > 20 and stats[0][7] > 0
    return _case([frame(pts((9, 8, 60), (8, 7, -40), (9, 9, 63), (10, 8, 63), (5, 6, -300), (11, 12, 400)), S8, (0, 0, 0))], dense(), enters)


def margins():
    """rays of m = 4 and m = 1 under the largest G, G > m, G = m, G = m - 1 = 3 and G = 0: each frame walks further than the one before"""
    def enters(case, stats):
        counts = [len(spans(case, k)[0]) for k in range(5)]
        return sorted(m for m, _ in lengths(case)) == [1, 4, 4] and counts == [0, 0, 0, 2, 9] and all(s[6:] == (3, 0, 0) for s in stats[:3]) and \
            stats[3][7] > 0 and stats[4][7] > 0
    rays = pts((12, 8, 30), (6, 4, 2), (8, 9, 20))
    return _case([frame(rays, S8, (G, 1, 0)) for G in (0xFFFFFFFF, 1000, 4, 3, 0)], full(), enters)


# ---- keep_ground --------------------------------------------------------------------------------------------------------------------
RAYS16 = pts((14, 8, 8), (13, 13, 30), (2, 8, 0), (8, 2, 63), (3, 3, 9), (9, 8, 20), (14, 14, -40), (2, 14, 3))


def keep_ground(keep):
    def build():
        def enters(case, stats):
            return stats[0][7] > 0 and (stats[0][8] == 0 if keep else stats[0][8] > 0)
        start = dense()
        start[::2, ::2] = U64(1) << U64(8)  # columns that are the sensor's slab alone: emptied unless the ground is kept
        return _case([frame(RAYS16, S8, (0, 1, keep))], start, enters)
    return build


def emptied_once_under_4096_rays():
    """4 096 points in one cell, their rays all through the sensor's cell and its diagonal neighbour; W = 64 clears both columns whole:
    each is emptied by exactly one of thousands of atomics"""
    def enters(case, stats):
        return stats[0][6] == 4096 and stats[0][8] == 2 and stats[0][7] == 64 + 3 and stats[1][6:] == (4096, 0, 0)
    start = zeros()
    start[8, 8], start[9, 9], start[10, 10] = U64(ec.FULL), U64(ec.bits(0, 31, 63)), U64(ec.bits(5))
    return _case([frame(ec.contended_one_cell(), S8, (0, 64, 0)), frame(ec.contended_one_cell(), S8, (0, 64, 0))], start, enters)


# ---- contention ---------------------------------------------------------------------------------------------------------------------
def contended_three_triples():
    def enters(case, stats):
        return len(ecr.triples(case["cfg"], *case["frames"][0][:3])[1]) == 3 and stats[0][6] == 4096 and stats[0][7] > 0 and stats[1][7] == 0
    return _case([frame(ec.contended_three(), ec.SENSOR16, (0, 1, 1)), frame(ec.contended_three(), ec.SENSOR16, (0, 1, 1))], full(), enters)


def contended_64_slabs_of_one_cell():
    def enters(case, stats):
        return len(ecr.triples(case["cfg"], *case["frames"][0][:3])[1]) == 64 and stats[0][6] == 4096 and stats[0][7] > 0
    return _case([frame(ec.contended_one_cell(), ec.SENSOR16, (0, 0, 0)), frame(ec.contended_one_cell(), ec.SENSOR16, (1, 1, 1))], dense(), enters)


def hit_wins():
    """returns that lie on other returns' rays - in line with the sensor, at its slab and on a slope - are all set after the update"""
    def enters(case, stats):
        after = reference_columns(case)[0]
        points, pose, sensor, (G, W, _) = case["frames"][0]
        _, gx, gy, mask = ecr.steps(case["cfg"], points, pose, sensor, G, W)
        carved = {(int(x), int(y)) for x, y, m in zip(gx, gy, mask) if int(m)}
        cls, cx, cy, s = er.point_classes(case["cfg"], points, pose, sensor)
        return (cls == er.USED).all() and sum((int(x), int(y)) in carved for x, y in zip(cx, cy)) >= 6 and \
            all((int(after[int(y), int(x)]) >> int(b)) & 1 for x, y, b in zip(cx, cy, s))
    line = pts((9, 8, 8), (10, 8, 8), (11, 8, 8), (12, 8, 8), (14, 8, 8), (9, 9, 12), (10, 10, 16), (11, 11, 20), (12, 12, 24), (13, 13, 28))
    return _case([frame(line, S8, (0, 1, 0))], full(), enters)


# ---- lanes striding: rays longer than a wave ---------------------------------------------------------------------------------------------
CFG140 = er.make_config(0.25, 0.0, 0.0, 140, 3, -1.0, 0.125, 35.0)  # reach 140


def long_rays():
    def enters(case, stats):
        return case["cfg"]["reach"] == 140 and sorted(m for m, _ in lengths(case)) == [63, 64, 65, 129] and stats[0][7] > 100
    sensor = at(5, 1, 8, CFG140)
    return _case([frame(pts((68, 1, 40), (69, 0, -10), (70, 2, 8), (134, 1, 70), cfg=CFG140), sensor, (2, 1, 1))], dense(CFG140), enters, CFG140)


# ---- the list's length around a wave, a wave's 256 points and a workgroup --------------------------------------------------------------------------------------
def list_of(n):
    def build():
        def enters(case, stats):
            return stats[0][6] == n and (n < 63 or stats[0][3] > 0)  # every point is listed, the OUTSIDE_COLUMN ones among them
        rng = np.random.default_rng(100 + n)
        points = np.concatenate([rng.uniform(-1.2, 1.4, (n, 2)), rng.uniform(-2.0, 8.0, (n, 1))], axis=1)
        return _case([frame(points, ec.SENSOR16, (1, 1, 1))], dense(), enters)
    return build


# ---- the edge of the grid ---------------------------------------------------------------------------------------------------------------
def sensor_outside_the_grid():
    """the sensor's cell (-2, 8) lies outside: the rays' first steps are ignored, the rest carve"""
    def enters(case, stats):
        sx, sy, ss = ecr.sensor(case["cfg"], *case["frames"][0][1:3])
        _, gx, gy, _ = ecr.steps(case["cfg"], *case["frames"][0][:3], 0, 1)
        return (sx, sy) == (-2, 8) and (gx < 0).any() and (gx >= 0).any() and stats[0][7] > 0
    return _case([frame(pts((4, 8, 8), (3, 13, 30), (0, 3, 2), (2, 8, 50)), at(-2, 8, 8), (0, 1, 1))], dense(), enters)


def endpoints_outside():
    """OUTSIDE_GRID endpoints (the sensor in cell (13, 8), endpoints in columns 16 .. 18) and OUTSIDE_COLUMN endpoints carve"""
    def enters(case, stats):
        return stats[0][:4] == (0, 0, 3, 2) and stats[0][6] == 5 and stats[0][7] > 0
    points = pts((17, 8, 8), (18, 11, 30), (16, 5, -3), (10, 8, 64), (13, 3, -1))
    return _case([frame(points, at(13, 8, 8), (0, 0, 1))], dense(), enters)


def nothing_finite():
    """a NaN pose and a NaN sensor: every point is skipped; a sensor whose slab is out of range: the points are used, nothing is carved;
    a NaN pose height: the plane is finite, every point skipped; and a frame of no points"""
    def enters(case, stats):
        return stats[0] == stats[1] == stats[3] == (0, 8, 0, 0, 0, 0, 0, 0, 0) and stats[2][0] == 7 and stats[2][6:] == (0, 0, 0) and stats[4] == (0,) * 9
    nan_pose, nan_z = np.array([0.0, 0.0, 0.0, 1.0, NAN, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, NAN])
    return _case([frame(RAYS16, S8, (0, 1, 0), pose=nan_pose), frame(RAYS16, [NAN, 0.1, 0.0], (0, 1, 0)), frame(RAYS16, [0.1, 0.1, 1.0e6], (0, 1, 0)),
                  frame(RAYS16, S8, (0, 1, 0), pose=nan_z), frame(np.zeros((0, 3)), S8, (0, 1, 0))], zeros(), enters)


# ---- a drive ----------------------------------------------------------------------------------------------------------------------------
def drive():
    """the six frames of elev_cases.random_drive() with G = 1, W = 1 and keep_ground set"""
    def enters(case, stats):
        return all(s[6] > 1000 and s[6] >= s[0] for s in stats) and any(s[6] > s[0] for s in stats) and all(s[7] > 100 for s in stats[1:5]) and \
            all(s[8] == 0 for s in stats)
    cfg, frames = ec.random_drive()
    return _case([(p, pose, sensor, (1, 1, 1)) for p, pose, sensor in frames], zeros(cfg), enters, cfg)


CASES = {
    "mask_reaching_bit_63": mask_reaching_bit_63, "mask_hi_64_and_above": mask_hi_64_and_above, "mask_lo_below_0": mask_lo_below_0,
    "spans_wholly_outside": spans_wholly_outside, "sensor_above_and_below_the_column": sensor_above_and_below_the_column,
    "widen_0": widen(0), "widen_1": widen(1), "widen_64": widen(64),
    "level_rays": level_rays, "steep_rays": steep_rays, "margins": margins,
    "keep_ground_set": keep_ground(1), "keep_ground_clear": keep_ground(0), "emptied_once_under_4096_rays": emptied_once_under_4096_rays,
    "contended_three_triples": contended_three_triples, "contended_64_slabs_of_one_cell": contended_64_slabs_of_one_cell, "hit_wins": hit_wins,
    "long_rays": long_rays,
    "list_of_1": list_of(1), "list_of_63": list_of(63), "list_of_64": list_of(64), "list_of_65": list_of(65), "list_of_257": list_of(257),
    "list_of_1025": list_of(1025),  # the listing kernel's second workgroup: a lane takes four points, a workgroup 1 024
    "sensor_outside_the_grid": sensor_outside_the_grid, "endpoints_outside": endpoints_outside, "nothing_finite": nothing_finite,
    "drive": drive,
}


def reference_columns(case):
    return reference_run(case)[0]


def reference_run(case):
    """-> (columns after every frame, the nine words of every frame) by the restatement"""
    columns = case["start"].copy()
    after, stats = [], []
    for points, pose, sensor, (G, W, keep) in case["frames"]:
        stats.append(ecr.update(case["cfg"], columns, points, pose, sensor, G, W, keep))
        after.append(columns.copy())
    return after, stats


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, columns after every frame, stats of every frame) - computed once per process, shared and left unchanged"""
    case = CASES[name]()
    after, stats = reference_run(case)
    return case, after, stats


def layer_config(cfg):
    """the fields of a kicp_elev_config"""
    return {k: cfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_origin", "slab", "max_ray")}


def write_case(path, case):
    """the input file of tests/cpp/elev_carve_host_test.cpp: doubles - cell, origin_x, origin_y, width, height, z_origin, slab, max_ray,
    frames; the start columns (uint64 per cell); then per frame pose[7], sensor[3], G, W, keep_ground, n and the n points"""
    cfg = case["cfg"]
    with open(path, "wb") as f:
        np.array([cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_origin"], cfg["slab"], cfg["max_ray"], len(case["frames"])],
                 dtype=np.float64).tofile(f)
        np.ascontiguousarray(case["start"], dtype=U64).tofile(f)
        for points, pose, sensor, (G, W, keep) in case["frames"]:
            np.concatenate([pose, sensor, [float(G), float(W), float(keep), float(len(points))]]).astype(np.float64).tofile(f)
            np.ascontiguousarray(points, dtype=np.float64).tofile(f)


# ---- the passer-by ------------------------------------------------------------------------------------------------------------------------
PASSER_CFG = er.make_config(0.1, -14.0, -14.0, 300, 300, -1.0, 0.0625, 25.0)
PASSER_CARVE = (2, 1, 1)
PASSER_CLASSES = (2, 28)
PASSER_REGION = (slice(142, 150), slice(158, 166))  # cells y 142 .. 149, x 158 .. 165: the box and a ring of two cells


@functools.lru_cache(maxsize=None)
def passer_by():
    """elev_cases.drive_scene()'s scene seen through 32 x 512 beams from four poses, a box of 0.4 x 0.4 x 1.7 m standing at x 2.0 .. 2.4,
    y 0.4 .. 0.8 in frames 0 and 1 only -> the frames (points in the base frame, pose, sensor)"""
    _, scene, _ = ec.drive_scene()
    with_box = syn.Scene(scene.half, scene.height, np.vstack([scene.boxes, [[2.0, 0.4, 0.0, 2.4, 0.8, 1.7]]]))
    dirs = syn.beam_directions(32, 512, (-25.0, 10.0))
    frames = []
    for k, (x, y) in enumerate([(0.0, 0.0), (0.2, 0.05), (0.4, 0.1), (0.6, 0.1)]):
        pose = gc.tilted_pose(x, y, 0.05 * k, 0, 0, z=0)
        world_from_lidar = syn.pose_mul(pose, ec.DRIVE_EXT)
        R = syn.quat_to_matrix(world_from_lidar[:4])
        t = (with_box if k < 2 else scene).raycast(world_from_lidar[4:], dirs @ R.T) + np.random.default_rng(k).normal(0, 0.01, len(dirs))
        frames.append((np.ascontiguousarray(syn.pose_act(ec.DRIVE_EXT, dirs * t[:, None])), pose, ec.DRIVE_EXT[4:].copy()))
    return frames


@functools.lru_cache(maxsize=None)
def passer_by_reference():
    """-> (columns under plain integration, columns under the update) after frame 3, by the restatements"""
    plain, carved = zeros(PASSER_CFG), zeros(PASSER_CFG)
    for points, pose, sensor in passer_by():
        er.integrate(PASSER_CFG, plain, points, pose, sensor)
        ecr.update(PASSER_CFG, carved, points, pose, sensor, *PASSER_CARVE)
    return plain, carved
