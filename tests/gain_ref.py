"""The information gain of include/kicp.h ("what the robot would see from there") restated in plain Python and numpy, from the header's
text and not from the C++: the classes, the 8 R offsets at Chebyshev distance R, the walk's closed form, the tests of one step in the
header's order, and the distinct cells through a boolean window.  Also the cases the test files share."""
import functools

import numpy as np

from frontier_ref import counts_of, random_occupancy  # noqa: F401 (the test files take them from here)

WORDS = 4
CLEAR, UNKNOWN, OCCUPIED = 0, 1, 2


def classes(occ, occupied_thresh=0.65):
    """int (H, W) of CLEAR / UNKNOWN / OCCUPIED: occupied when (double)v > occupied_thresh * 100.0, else unknown when v < 0"""
    occ = np.asarray(occ, dtype=np.int8)
    occupied = occ.astype(np.float64) > occupied_thresh * 100.0
    return np.where(occupied, OCCUPIED, np.where(occ < 0, UNKNOWN, CLEAR))


def perimeter(R):
    """the 8 R offsets (dx, dy) with max(|dx|, |dy|) == R, each once - in no particular order: the result does not depend on it"""
    return [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if max(abs(dx), abs(dy)) == R]


def step(dx, dy, R, k):
    """the offset of step k of the walk to (dx, dy) with m = R"""
    sa, sb = (2 * k * abs(dx) + R) // (2 * R), (2 * k * abs(dy) + R) // (2 * R)
    return (-sa if dx < 0 else sa), (-sb if dy < 0 else sb)


def gain_one(cls, vx, vy, R, visits=None):
    """one viewpoint on a class plane (a list of lists) -> [seen, blocked, left, class]; visits: a list that takes the offset of every visit inside the disc"""
    H, W = len(cls), len(cls[0])
    own = cls[vy][vx]
    if own != CLEAR:
        return [0, 0, 0, own]
    window = np.zeros((2 * R + 1, 2 * R + 1), dtype=bool)
    blocked = left = 0
    for dx, dy in perimeter(R):
        for k in range(1, R + 1):
            ox, oy = step(dx, dy, R, k)
            if ox * ox + oy * oy > R * R:
                break
            if visits is not None:
                visits.append((ox, oy))
            x, y = vx + ox, vy + oy
            if not (0 <= x < W and 0 <= y < H):
                left += 1
                break
            if cls[y][x] == OCCUPIED:
                blocked += 1
                break
            if cls[y][x] == UNKNOWN:
                window[oy + R, ox + R] = True
    return [int(window.sum()), blocked, left, own]


def as_indices(views, width):
    v = np.asarray(views, dtype=np.int64)
    return (v[:, 1] * width + v[:, 0]) if v.ndim == 2 else v


def gain(occ, views, R, occupied_thresh=0.65):
    """-> uint32 (N, 4); views: cell indices or (N, 2) of (x, y)"""
    cls = classes(occ, occupied_thresh).tolist()
    W = len(cls[0])
    return np.array([gain_one(cls, int(c) % W, int(c) // W, R) for c in as_indices(views, W)], dtype=np.uint32).reshape(-1, WORDS)


def from_text(rows):
    """rows of digits, y = 0 first: 0 clear, 1 unknown, 2 occupied -> a readout"""
    value = {"0": 0, "1": -1, "2": 100}
    return np.array([[value[ch] for ch in row] for row in rows], dtype=np.int8)


def pinned_9x7():
    """include/kicp.h's example -> (readout, viewpoints (x, y), {R: rows})"""
    occ = from_text(["111111111", "100000211", "100020111", "100000011", "120000001", "100000001", "111111111"])
    views = [(3, 3), (1, 1), (7, 5), (4, 2), (0, 0)]
    want = {1: [[0, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 2], [0, 0, 0, 1]],
            2: [[0, 3, 0, 0], [5, 0, 2, 0], [6, 0, 2, 0], [0, 0, 0, 2], [0, 0, 0, 1]],
            3: [[3, 5, 0, 0], [7, 1, 13, 0], [9, 0, 13, 0], [0, 0, 0, 2], [0, 0, 0, 1]],
            4: [[15, 7, 3, 0], [9, 2, 21, 0], [13, 0, 21, 0], [0, 0, 0, 2], [0, 0, 0, 1]]}
    return occ, views, {R: np.array(rows, dtype=np.uint32) for R, rows in want.items()}


# the visits of the 8 R rays on an empty plane, those the disc test ends left out (include/kicp.h)
EMPTY_PLANE_VISITS = {1: 4, 2: 20, 3: 52, 7: 316, 20: 2736, 64: 28596, 65: 29512, 100: 70096}


def edge_views(width, height):
    """the four corners and the middles of the four edges, as (x, y)"""
    xs, ys = sorted({0, width // 2, width - 1}), sorted({0, height // 2, height - 1})
    return [(x, y) for y in ys for x in xs if x in (0, width - 1) or y in (0, height - 1)]


def spread_views(occ, n, seed):
    """n cell indices drawn over the whole grid: clear, unknown and occupied cells mixed, as they come"""
    return np.random.default_rng(seed).integers(0, occ.size, n).astype(np.uint32)


def cases():
    """name -> (readout int8 (H, W), viewpoints, [R, ..]): the issue's list.  The reference walks every ray in Python, so the large R
    come with few viewpoints and the many viewpoints with small R."""
    out = {}
    occ, views, _ = pinned_9x7()
    out["pinned_9x7"] = (occ, views, [1, 2, 3, 4])
    # R at a wave's trip boundary and beyond, on a random grid: viewpoints in the middle, at the corners and on the edges
    occ = random_occupancy(130, 100, 11)
    occ[45:56, 60:71] = 0  # clear round the middle viewpoints, so that their rays start
    out["random_130x100_trips"] = (occ, [(65, 50), (64, 49)] + edge_views(130, 100), [63, 64, 65])
    out["random_130x100_r128"] = (occ, [(65, 50), (0, 0), (129, 99)], [128])
    out["random_130x100_small_r"] = (occ, [(65, 50), (61, 46), (70, 55)] + edge_views(130, 100), [1, 2, 5])
    occ = random_occupancy(70, 50, 3)
    occ[0, 0] = occ[0, 69] = occ[49, 0] = occ[49, 69] = occ[25, 35] = 0
    out["random_70x50"] = (occ, [(35, 25)] + edge_views(70, 50), [1, 7, 20, 64])
    # the LDS cap: one viewpoint, most rays LEFT
    occ = random_occupancy(40, 40, 5, unknown=0.5, occupied=0.02)
    occ[18:23, 18:23] = 0
    out["cap_361_in_40x40"] = (occ, [(20, 20)], [361])
    out["one_cell_clear"] = (np.zeros((1, 1), dtype=np.int8), [0], [1, 2, 64])
    out["one_cell_unknown"] = (np.full((1, 1), -1, dtype=np.int8), [0], [1, 3])
    occ = random_occupancy(1, 70, 77, unknown=0.4, occupied=0.05)
    occ[[0, 35, 69], 0] = 0
    out["random_1x70"] = (occ, [0, 35, 69, 10, 50], [1, 2, 30, 64, 65, 100])
    out["all_unknown"] = (np.full((35, 40), -1, dtype=np.int8), [(0, 0), (20, 17), (39, 34)], [1, 20])
    out["all_clear"] = (np.zeros((35, 40), dtype=np.int8), [(0, 0), (20, 17), (39, 34), (39, 0)], [1, 10, 20, 64])
    out["all_occupied"] = (np.full((35, 40), 100, dtype=np.int8), [(0, 0), (20, 17)], [1, 20])
    # a clear viewpoint inside rings of unknown cells at distance 1 and 2, which many rays cross
    occ = np.zeros((41, 41), dtype=np.int8)
    occ[18:23, 18:23] = -1
    occ[20, 20] = 0
    out["unknown_rings"] = (occ, [(20, 20)], [1, 2, 3, 10, 20])
    # occupied cells exactly on the disc's edge, and one just beyond it, at R = 5; unknown everywhere else but round the viewpoint
    for name, cells in (("disc_edge_5_0", [(5, 0)]), ("disc_edge_3_4", [(3, 4)]), ("disc_beyond_4_4", [(4, 4)]), ("disc_edge_all", [(5, 0), (3, 4), (4, 4), (-4, -3), (0, -5)])):
        occ = np.full((31, 31), -1, dtype=np.int8)
        occ[13:18, 13:18] = 0
        for ox, oy in cells:
            occ[15 + oy, 15 + ox] = 100
        out[name] = (occ, [(15, 15)], [5, 4, 6])
    # a wall one cell thick, and a diagonal one whose cells touch at corners only: rays may slip through it
    occ = np.zeros((50, 60), dtype=np.int8)
    occ[:, 40:] = -1
    occ[5:45, 35] = 100
    out["thin_wall"] = (occ, [(20, 25), (34, 25), (36, 25), (20, 2)], [10, 25, 40])
    occ = np.zeros((60, 60), dtype=np.int8)
    yy, xx = np.mgrid[0:60, 0:60]
    occ[xx + yy > 70] = -1
    occ[(xx + yy == 70) & (xx > 15) & (xx < 55)] = 100
    out["diagonal_wall"] = (occ, [(25, 25), (30, 30), (34, 35), (20, 40)], [12, 30, 45])
    # an unknown region behind an occupied cell: shadowed
    occ = np.zeros((41, 61), dtype=np.int8)
    occ[:, 30:] = -1
    occ[18:23, 25] = 100
    out["shadow"] = (occ, [(20, 20), (23, 20), (20, 5)], [15, 30])
    # many viewpoints: more workgroups than CUs, duplicates, unknown and occupied cells mixed in
    occ = random_occupancy(70, 50, 21)
    views = spread_views(occ, 300, 4)
    views[100:110] = views[0:10]
    out["random_70x50_300_views"] = (occ, views, [6])
    occ = random_occupancy(130, 100, 22)
    out["random_130x100_views"] = (occ, spread_views(occ, 40, 5), [20])
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """(name, R) -> the rows of cases() by this restatement: computed once per process, shared by the test files, read-only"""
    out = {}
    for name, (occ, views, ranges) in cases().items():
        for R in ranges:
            out[(name, R)] = gain(occ, views, R)
            out[(name, R)].setflags(write=False)
    return out
