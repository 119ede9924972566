"""The case table of the occupancy grid's regime tests, shared by tests/test_plan_cases.py (CPU: the premises of every case, from
numpy and the restatements alone) and tests/test_gpu_plan_regimes.py (GPU: kicp_nav.hpp k_nav_goals and k_nav_count, kicp_clear.hpp
k_clear_columns and k_clear_rows, kicp_elev.hpp k_elev_mark, k_elev_classify and k_elev_to_grid).  Nothing here calls the GPU or the
library: only numpy and potential_ref, clearance_ref, elev_ref, elev_cases.

Every regime follows from a case's shape by the arithmetic stated next to it (goals per workgroup, lanes of the counting launch,
waves per shard); the constants below restate the kernels' launch shapes as the cases were chosen for, and the CPU test checks the
cases against them, never the library against them.

Potential:  257 goals (a second workgroup with one live lane), 600 goals (duplicates, impassable ones, 40 in one tile), every cell a
goal (16 workgroups), 1 030 x 260 cells (the counting launch's second trip), and the small map on the large map's handle.
Clearance:  3 x 520 and 520 x 3 with two sources at R = 254 and R = 253 (column distances 253, 254 and "none" side by side, sweeps
that run more than 255 rows past their source, row scans to k = 254), 300 x 300 with 0.05 % sources at R = 254.
Height columns:  layers with sides 1, 15 .. 17, 31 .. 33 and 40; 300 x 300 random columns and the columns of a drive (1 444 waves on
64 shards); frames of 63 .. 257 points and one of 20 000."""
import functools

import numpy as np

import clearance_ref as cr
import elev_cases as ec
import elev_ref as er
import potential_ref as pr

U64 = np.uint64


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- potential ---------------------------------------------------------------------------------------------------------------------
NAV_TILE = 32                 # cells per side of a relaxation tile
NAV_GOAL_LANES = 256          # goals per workgroup of the goal launch
NAV_COUNT_LANES = 1024 * 256  # lanes of the counting launch: a grid with more cells needs a second trip


def tile_of(x, y, width):
    return (y // NAV_TILE) * (-(-width // NAV_TILE)) + x // NAV_TILE


@functools.lru_cache(maxsize=None)
def map_96x70():
    """the random 96 x 70 costmap of the goal cases, 30 % impassable; 3 x 3 tiles, the far corner tile is x 64 .. 95, y 64 .. 69"""
    cm = pr.random_costmap(96, 70, 41)
    cm[66, 90] = 200  # the cell of goal 257
    return frozen(cm)


@functools.lru_cache(maxsize=None)
def goals_257():
    """256 goals drawn from all cells outside the far corner tile, then (90, 66): the one goal of the second workgroup and the only
    goal of its tile"""
    rng = np.random.default_rng(42)
    goals = []
    while len(goals) < 256:
        x, y = int(rng.integers(0, 96)), int(rng.integers(0, 70))
        if not (x >= 64 and y >= 64):
            goals.append((x, y))
    return tuple(goals) + ((90, 66),)


ONE_TILE = (32, 32, 32, 32)  # the middle tile of the 96 x 70 map as x0, y0, w, h


@functools.lru_cache(maxsize=None)
def goals_600():
    """510 cells drawn from all cells of the map (about 30 % impassable), 40 more inside ONE_TILE, then 50 of those 550 again; shuffled"""
    rng = np.random.default_rng(43)
    goals = [(int(rng.integers(0, 96)), int(rng.integers(0, 70))) for _ in range(510)]
    goals += [(int(rng.integers(32, 64)), int(rng.integers(32, 64))) for _ in range(40)]
    goals += [goals[k] for k in rng.choice(550, 50, replace=False)]
    return tuple(goals[k] for k in rng.permutation(600))


@functools.lru_cache(maxsize=None)
def map_65x63():
    return frozen(pr.random_costmap(65, 63, 44))


def goals_every_cell(width, height):
    return tuple((x, y) for y in range(height) for x in range(width))


LARGE_W, LARGE_H = 1030, 260  # 267 800 cells, 33 x 9 tiles with partial tiles on both axes
LARGE_GOAL = (5, 0)
LARGE_CLAMP = 4000


@functools.lru_cache(maxsize=None)
def map_large():
    """mostly impassable, so that the restatement stays cheap: a column at x = 5 (q = 3) joins three rows at the bottom (q = 2) to ten
    rows at the top (q = 7); the top rows hold the flat indices from 257 500 on, the column crosses index 262 144 on its way"""
    cm = np.zeros((LARGE_H, LARGE_W), dtype=np.uint8)
    cm[:, 5] = 3
    cm[0:3, :] = 2
    cm[250:260, :] = 7
    return frozen(cm)


# the same map from COUNTERS: impassable cells are sources, the top rows unknown, everything else clear; at R = 1 the table gives a
# clear cell beside a source the cost 1 and every other clear cell 0, and the weights turn 0, 1 and "unknown" into q = 2, 3 and 7.  So
# the column has q = 3 again, the bottom rows 2 (row 2, beside the sources of row 3: 3), the top rows 7.
LARGE_TABLE = np.array([254, 1, 0], dtype=np.uint8)
LARGE_WEIGHT = np.zeros(256, dtype=np.uint8)
LARGE_WEIGHT[0], LARGE_WEIGHT[1], LARGE_WEIGHT[255] = 2, 3, 7
frozen(LARGE_TABLE, LARGE_WEIGHT)


@functools.lru_cache(maxsize=None)
def occupancy_large():
    """-> (occ int8, the restatement's costmap of it at LARGE_TABLE)"""
    cm = map_large()
    occ = np.where(cm > 0, 0, 100).astype(np.int8)
    occ[250:260, :] = -1
    costmap = cr.costmap(occ, LARGE_TABLE, clear=cr.clearance_by_offsets(occ, 1))
    return frozen(occ, costmap)


def embedded_small():
    """the 96 x 70 map in the corner of an otherwise impassable 1 030 x 260 costmap (tiles coincide): the small call a large grid's
    handle takes after the large one"""
    cm = np.zeros((LARGE_H, LARGE_W), dtype=np.uint8)
    cm[:70, :96] = map_96x70()
    return cm


def beyond_one_trip(pot, max_potential):
    """(cells below, cells equal) among the flat indices a single trip of the counting launch never reads"""
    tail = pot.ravel()[NAV_COUNT_LANES:]
    return int((tail < max_potential).sum()), int((tail == max_potential).sum())


# ---- clearance ---------------------------------------------------------------------------------------------------------------------
CLEAR_STRIP = 254  # rows of a column strip at R >= 32: max(32, R)


@functools.lru_cache(maxsize=None)
def tall_3x520():
    """three columns, 520 rows: sources at (0, 0) and (2, 519) only, one unknown cell at (1, 300) - a third source when unknown cells
    are obstacles, and 219 rows from a source, where the table still has a cost for it, when they are not"""
    occ = np.zeros((520, 3), dtype=np.int8)
    occ[0, 0] = occ[519, 2] = 100
    occ[300, 1] = -1
    return frozen(occ)


@functools.lru_cache(maxsize=None)
def wide_520x3():
    return frozen(np.ascontiguousarray(tall_3x520().T))


@functools.lru_cache(maxsize=None)
def sparse_300():
    """300 x 300, 0.05 % sources and as few unknown cells, kept only in the 50 columns on the left and the 20 rows on top: the rest
    of the grid lies up to 250 cells from them, so most scans run far and some the full radius"""
    occ = cr.random_occupancy(300, 300, 0.0005, 45, unknown_fraction=0.0005)
    inner = occ[:280, 50:]
    inner[(inner > 65) | (inner < 0)] = 30
    return frozen(occ)


# name -> (occupancy, R, rectangles): strips whose run-in clips at neither end, at one end and at both; single cells at the rows
# (columns) 254 and 255, where 254^2 and "far" are neighbours
def clearance_cases():
    tall = [None, (0, 254, 3, 2), (1, 200, 1, 120), (0, 254, 1, 1), (0, 255, 1, 1), (2, 265, 1, 1), (2, 264, 1, 1), (0, 300, 3, 10), (1, 100, 2, 20)]
    wide = [None, (254, 0, 2, 3), (255, 1, 120, 1), (256, 0, 1, 1), (254, 0, 1, 1), (255, 0, 1, 1), (265, 2, 1, 1), (200, 1, 120, 1)]
    return {
        "tall_3x520_r254": (tall_3x520(), 254, tall),
        "wide_520x3_r254": (wide_520x3(), 254, wide),
        "tall_3x520_r253": (tall_3x520(), 253, tall),
        "wide_520x3_r253": (wide_520x3(), 253, wide),
        "sparse_300x300_r254": (sparse_300(), 254, [None, (20, 30, 260, 240)]),
    }


@functools.lru_cache(maxsize=None)
def clearance_of(name, unknown_is_obstacle):
    """the restatement's full-grid clearance of a case, computed once"""
    occ, radius, _ = clearance_cases()[name]
    return frozen(cr.clearance(occ, radius, unknown_is_obstacle=unknown_is_obstacle))


# ---- height columns ----------------------------------------------------------------------------------------------------------------
ELEV_TILE = 16
ELEV_SHARDS = 64
SMALL_LAYERS = [(1, 1), (1, 40), (40, 1), (15, 17), (16, 16), (17, 15), (31, 33), (32, 32), (33, 31)]  # (width, height)
LOW, HIGH = ec.bits(3), ec.bits(30)  # two grounds 27 slabs apart: a STEP at every S of ec.PARAMS but 62


def sparse_columns(width, height, seed):
    """ec.random_columns("sparse") at another shape: two random bits in 60 % of the cells, the rest unknown"""
    rng = np.random.default_rng(seed)
    few = (U64(1) << rng.integers(0, 64, (height, width), dtype=U64)) | (U64(1) << rng.integers(0, 64, (height, width), dtype=U64))
    return few * (rng.random((height, width)) < 0.6).astype(U64)


def wrap_bait(width, height):
    """(x, y) of the hand-placed cell in the layer's last column that is traversable, and would be a STEP if the cell beyond the
    row's end were read from the next row's first column; None where the layer has no room for it"""
    return (width - 1, 8) if width >= 15 and height >= 11 else None


def small_layer_columns(width, height):
    """random sparse columns with a hand-placed STEP pair across every tile border of the full layer, the higher cell on either side,
    one at every grid corner, and the wrap bait"""
    c = sparse_columns(width, height, 1000 * width + height)
    for x in range(ELEV_TILE - 1, width - 1, ELEV_TILE):  # vertical borders, at rows 2 and 4 (or the layer's only row)
        for y, (a, b) in zip((2, 4) if height > 4 else (0,), ((LOW, HIGH), (HIGH, LOW))):
            c[y, x], c[y, x + 1] = a, b
    for y in range(ELEV_TILE - 1, height - 1, ELEV_TILE):  # horizontal borders, at columns 2 and 5 (or the only column)
        for x, (a, b) in zip((2, 5) if width > 5 else (0,), ((LOW, HIGH), (HIGH, LOW))):
            c[y, x], c[y + 1, x] = a, b
    if width >= 2 and height >= 2:  # each grid corner is the higher cell of a diagonal pair
        for x, y, nx, ny in ((0, 0, 1, 1), (width - 1, 0, width - 2, 1), (0, height - 1, 1, height - 2), (width - 1, height - 1, width - 2, height - 2)):
            c[y, x], c[ny, nx] = ec.bits(20), ec.bits(1)
    elif width * height > 1:  # a layer one cell wide: both ends
        flat = c.reshape(-1)
        flat[0], flat[1], flat[-1], flat[-2] = ec.bits(20), ec.bits(1), ec.bits(20), ec.bits(1)
    bait = wrap_bait(width, height)
    if bait:
        x, y = bait
        c[y - 1:y + 2, x - 1:x + 1] = 0
        c[y, x] = HIGH
        c[y + 1, 0] = LOW
    return frozen(c)


def small_layer_rects(width, height):
    """the full layer, a rectangle from (1, 1) and one from (2, 3) whose last tiles overhang the layer, where they fit"""
    rects = [None]
    if width >= 3 and height >= 3:
        rects.append((1, 1, width - 1, height - 1))
    if width >= 4 and height >= 5:
        rects.append((2, 3, width - 2, height - 3))
    if height == 1 and width > 4:
        rects.append((3, 0, width - 3, 1))
    if width == 1 and height > 4:
        rects.append((0, 3, 1, height - 3))
    return rects


def classify_wrapped(columns, S, H):
    """the classes of a kernel whose halo guard admits x == width: the cell beyond a row's end reads the next row's first column"""
    height, width = columns.shape
    wide = np.zeros((height, width + 1), dtype=U64)
    wide[:, :width] = columns
    wide[:-1, width] = columns[1:, 0]
    return er.classify(wide, S, H)[0][:, :width]


BIG_RECT = (3, 5, 290, 280)


@functools.lru_cache(maxsize=None)
def columns_300():
    """300 x 300 random sparse columns, and 150 hand-made pairs that make BODY and STEP cells at (S, H) = (62, 63) too: a column of
    bits 0 and 63 (bit 63 is the one bit in (0 + 62, 0 + 63]), and a ground at 63 beside one at 0"""
    c = sparse_columns(300, 300, 46)
    rng = np.random.default_rng(47)
    for k in range(150):
        x, y = int(rng.integers(4, 290)), int(rng.integers(6, 280))
        c[y, x], c[y, x + 1] = ec.bits(0, 63), (ec.bits(63) if k % 2 else ec.bits(0))
    return frozen(c)


@functools.lru_cache(maxsize=None)
def drive_columns():
    """-> (cfg, frames, the columns the restatement has after the last frame of ec.random_drive())"""
    cfg, frames = ec.random_drive()
    after, _ = ec.reference_run(cfg, frames)
    return cfg, frames, frozen(after[-1])


@functools.lru_cache(maxsize=None)
def classified(which, S, H):
    """er.classify of columns_300() or the drive's columns, computed once per (S, H)"""
    columns = columns_300() if which == "random" else drive_columns()[2]
    return frozen(*er.classify(columns, S, H))


def shard_table(classes, body, rect=None):
    """What each of the 64 count shards receives when the classification of `rect` runs one wave per four rows of a 16 x 16 tile,
    wave w of tile t adding to shard (4 t + w) % 64 -> (sums int64 [64, 4], waves with something to add int64 [64, 4])"""
    H, W = classes.shape
    x0, y0, w, h = rect or (0, 0, W, H)
    which = np.where(classes == -1, 0, np.where(classes == 0, 1, np.where(body, 2, 3)))[y0:y0 + h, x0:x0 + w]
    tiles_x = -(-w // ELEV_TILE)
    sums, waves = np.zeros((ELEV_SHARDS, 4), dtype=np.int64), np.zeros((ELEV_SHARDS, 4), dtype=np.int64)
    for t in range(tiles_x * (-(-h // ELEV_TILE))):
        bx, by = (t % tiles_x) * ELEV_TILE, (t // tiles_x) * ELEV_TILE
        for wave in range(4):
            part = np.bincount(which[by + 4 * wave:by + 4 * wave + 4, bx:bx + ELEV_TILE].ravel(), minlength=4)
            sums[(4 * t + wave) % ELEV_SHARDS] += part
            waves[(4 * t + wave) % ELEV_SHARDS] += part > 0
    return sums, waves


FRAME_SIZES = [63, 64, 65, 255, 256, 257]  # around a wave and around a workgroup of the marking launch


@functools.lru_cache(maxsize=None)
def short_frames():
    """name -> (points, pose, sensor) on ec.CFG16: the first n points of ec.contended_three (three bits, every lane racing for them)
    and of ec.tilted_frame (all four classes of a point)"""
    tilted, pose, sensor = ec.tilted_frame()
    three = ec.contended_three()
    out = {}
    for n in FRAME_SIZES:
        out["contended_%d" % n] = (frozen(three[:n].copy()), ec.IDENTITY, ec.SENSOR16)
        out["tilted_%d" % n] = (frozen(tilted[:n].copy()), pose, sensor)
    return out


@functools.lru_cache(maxsize=None)
def long_frame(n=20000, seed=48):
    """ec.tilted_frame's 3 000 points tiled to n with a jitter of a few centimetres: 313 waves on 64 shards"""
    tilted, pose, sensor = ec.tilted_frame()
    rng = np.random.default_rng(seed)
    pts = np.tile(tilted, (-(-n // len(tilted)), 1))[:n] + rng.normal(0.0, 0.03, (n, 3))
    return frozen(np.ascontiguousarray(pts)), pose, sensor
