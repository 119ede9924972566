"""The exploration frontiers of include/kicp.h ("where to go while mapping") restated in plain Python and numpy: the classes and the
frontier-cell predicate with shifted arrays, the components by a breadth-first flood fill in ascending index order - and, independently,
by numpy min-label sweeps to a fixed point, which must agree - and the ten words per frontier from the labelled cells."""
from collections import deque

import numpy as np

NONE = 0xFFFFFFFF
WORDS = 10


def classes(occ, occupied_thresh=0.65):
    """-> (occupied, unknown, clear) as bool arrays of occ's shape"""
    occ = np.asarray(occ, dtype=np.int8)
    occupied = occ.astype(np.float64) > occupied_thresh * 100.0
    unknown = occ < 0
    return occupied, unknown, ~occupied & ~unknown


def frontier_cells(occ, occupied_thresh=0.65):
    """clear cells with an unknown edge neighbour inside the grid: outside is not unknown"""
    _, unknown, clear = classes(occ, occupied_thresh)
    u = np.zeros((unknown.shape[0] + 2, unknown.shape[1] + 2), dtype=bool)
    u[1:-1, 1:-1] = unknown
    return clear & (u[1:-1, :-2] | u[1:-1, 2:] | u[:-2, 1:-1] | u[2:, 1:-1])


def labels_flood(flags):
    """uint32 (H, W): the cells in ascending index order, each unlabelled frontier cell the seed of a breadth-first fill over the eight
    neighbours - the seed is its component's least index"""
    H, W = flags.shape
    f = flags.tolist()
    labels = [[NONE] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            if not f[y][x] or labels[y][x] != NONE:
                continue
            label = y * W + x
            labels[y][x] = label
            queue = deque([(x, y)])
            while queue:
                cx, cy = queue.popleft()
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        nx, ny = cx + dx, cy + dy
                        if 0 <= nx < W and 0 <= ny < H and f[ny][nx] and labels[ny][nx] == NONE:
                            labels[ny][nx] = label
                            queue.append((nx, ny))
    return np.array(labels, dtype=np.uint32).reshape(H, W)


def labels_sweeps(flags):
    """the same labels as the least fixed point of label(c) = min over c and its frontier neighbours, swept over the whole grid"""
    H, W = flags.shape
    big = np.int64(NONE)
    lab = np.full((H + 2, W + 2), big, dtype=np.int64)
    inner = lab[1:-1, 1:-1]
    inner[flags] = (np.arange(H * W, dtype=np.int64).reshape(H, W))[flags]
    while True:
        best = inner.copy()
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                np.minimum(best, lab[dy:dy + H, dx:dx + W], out=best)
        best[~flags] = big
        if np.array_equal(best, inner):
            return inner.astype(np.uint32)
        inner[...] = best


def rows_of(labels, potential=None, min_size=1):
    """uint64 (F, 10) from a label plane: label, size, sum x, sum y, min x, max x, min y, max y, and the least key pot * 2^32 + index
    split into best_potential and best_cell; frontiers below min_size dropped, ascending labels"""
    H, W = labels.shape
    ys, xs = np.nonzero(labels != NONE)
    members = {}
    for x, y in zip(xs.tolist(), ys.tolist()):
        members.setdefault(int(labels[y, x]), []).append((x, y))
    out = []
    for label in sorted(members):
        cells = members[label]
        if len(cells) < min_size:
            continue
        key = min(((int(potential[y, x]) if potential is not None else NONE) << 32) + y * W + x for x, y in cells)
        cx, cy = [c[0] for c in cells], [c[1] for c in cells]
        out.append([label, len(cells), sum(cx), sum(cy), min(cx), max(cx), min(cy), max(cy), key >> 32, key & 0xFFFFFFFF])
    return np.array(out, dtype=np.uint64).reshape(-1, WORDS)


def frontiers(occ, occupied_thresh=0.65, min_size=1, potential=None):
    """-> (rows uint64 (F, 10), labels uint32 (H, W))"""
    labels = labels_flood(frontier_cells(occ, occupied_thresh))
    return rows_of(labels, potential, min_size), labels


def pinned_8x6():
    """An 8 x 6 readout with its frontier cells, labels and rows written out by hand; row y = 5 on top.  `.` clear (0), `u` unknown
    (-1), `S` occupied (100), `f` clear although busy (60 is not above 65).  On the right the frontier cells: A and B are the two
    frontiers, everything joined through corners.
        y 5   u u . . . . . .          - - B - - - - -
        y 4   u . . . . . S .          - B - - - - - A
        y 3   . . . S . . . u          B - - - - - A -
        y 2   . . . . . . u u          - - - - - A - -
        y 1   . f . . . . . u          - - - - A - A -
        y 0   . . . . u . . .          - - - A - A - A
    A = cells 3, 5, 7, 12, 14, 21, 30, 39 (label 3), B = cells 24, 33, 42 (label 24).
    -> (occ, labels, rows without a potential)"""
    text = ["....u...", ".f.....u", "......uu", "...S...u", "u.....S.", "uu......"]  # y = 0 first
    value = {".": 0, "u": -1, "S": 100, "f": 60}
    occ = np.array([[value[ch] for ch in row] for row in text], dtype=np.int8)
    labels = np.full(48, NONE, dtype=np.uint32)
    labels[[3, 5, 7, 12, 14, 21, 30, 39]] = 3
    labels[[24, 33, 42]] = 24
    rows = np.array([[3, 8, 3 + 5 + 7 + 4 + 6 + 5 + 6 + 7, 0 + 0 + 0 + 1 + 1 + 2 + 3 + 4, 3, 7, 0, 4, NONE, 3],
                     [24, 3, 0 + 1 + 2, 3 + 4 + 5, 0, 2, 3, 5, NONE, 24]], dtype=np.uint64)
    return occ, labels.reshape(6, 8), rows


def random_occupancy(width, height, seed, unknown=0.3, occupied=0.1):
    rng = np.random.default_rng(seed)
    occ = rng.integers(0, 66, (height, width)).astype(np.int8)
    u = rng.random((height, width))
    occ[u < unknown] = -1
    occ[u > 1.0 - occupied] = 100
    return occ


def in_unknown(width, height, cells):
    """unknown space with the listed cells (x, y) clear: each of them is a frontier cell unless clear cells surround it"""
    occ = np.full((height, width), -1, dtype=np.int8)
    for x, y in cells:
        occ[y, x] = 0
    return occ


def serpentine(width=130, height=100):
    """a corridor one cell wide through unknown space: a full row on every fourth row, joined at alternating ends - ONE thin frontier
    that runs through many tiles and re-enters them"""
    cells = []
    for k, y in enumerate(range(1, height - 1, 4)):
        cells += [(x, y) for x in range(1, width - 1)]
        if y + 4 < height - 1:
            cells += [((width - 2) if k % 2 == 0 else 1, y + d) for d in (1, 2, 3)]
    return in_unknown(width, height, cells)


def checkerboard(side=65):
    yy, xx = np.mgrid[0:side, 0:side]
    return np.where((xx + yy) % 2 == 0, 0, -1).astype(np.int8)


def diamond_ring(width=96, height=80, cx=48, cy=40, r=20):
    """cells with |x - cx| + |y - cy| = r: joined through corners only; its least index is the lower apex, in a tile of its own, and
    the row-major scan of every other tile meets the ring somewhere else"""
    yy, xx = np.mgrid[0:height, 0:width]
    return np.where(np.abs(xx - cx) + np.abs(yy - cy) == r, 0, -1).astype(np.int8)


def u_shape(width=70, height=50):
    """two arms that join only at the top: a row-major scan labels them apart first"""
    return in_unknown(width, height, [(10, y) for y in range(5, 41)] + [(50, y) for y in range(3, 41)] + [(x, 40) for x in range(10, 51)])


def cases():
    """name -> readout (int8 (H, W)): the issue's list"""
    out = {"pinned_8x6": pinned_8x6()[0]}
    for k, (w, h) in enumerate([(31, 31), (32, 32), (33, 33), (63, 65), (64, 64), (65, 63), (31, 64), (64, 33)]):
        out["random_%dx%d" % (w, h)] = random_occupancy(w, h, 100 + k)
    for w, h in ((1, 1), (1, 70), (70, 1)):
        out["random_%dx%d" % (w, h)] = random_occupancy(w, h, 7 * w + h, unknown=0.4)
    out["one_cell_clear"] = np.zeros((1, 1), dtype=np.int8)
    out["all_unknown"] = np.full((35, 40), -1, dtype=np.int8)
    out["all_clear"] = np.zeros((35, 40), dtype=np.int8)  # the cells on the grid's edge too: outside is not unknown
    out["all_occupied"] = np.full((35, 40), 100, dtype=np.int8)
    out["single_clear_cell"] = in_unknown(40, 40, [(20, 20)])
    out["corner_pair_31_31_32_32"] = in_unknown(64, 64, [(31, 31), (32, 32)])
    out["corner_pair_32_31_31_32"] = in_unknown(64, 64, [(32, 31), (31, 32)])
    out["two_apart"] = in_unknown(64, 64, [(30, 31), (32, 31), (10, 10), (10, 12), (40, 40), (42, 42)])
    out["along_a_tile_border"] = in_unknown(70, 70, [(x, y) for x in range(5, 61) for y in (31, 32)] + [(x, y) for y in range(40, 66) for x in (31, 32)])
    out["serpentine_130x100"] = serpentine()
    out["checkerboard_65"] = checkerboard()
    out["diamond_ring"] = diamond_ring()
    out["u_shape"] = u_shape()
    for seed in (1, 2, 3):
        out["random_70x50_seed%d" % seed] = random_occupancy(70, 50, seed)
        out["random_130x100_seed%d" % seed] = random_occupancy(130, 100, 10 + seed)
    return out


def room_drive(n=1500):
    """A short drive through a room of 12 m x 9 m with a pillar, on a 260 x 200 grid of 0.1 m cells with a 6 m sensor: per place a fan
    of n rays cast at the walls, yaw 0.  Walls farther than the sensor reaches stay unseen, so the seen floor ends in frontiers.
    -> (configuration as K.OccupancyGrid's arguments, [(points in the base frame, pose, sensor), ...], the places in metres)"""
    places = [(-3.0, -2.0), (-1.5, -1.0), (0.0, 0.5), (1.5, 1.0), (2.5, 1.2)]
    sensor = np.array([0.2, 0.0, 0.4])
    az = np.linspace(-np.pi, np.pi, n, endpoint=False) + 1e-3
    c, s = np.cos(az), np.sin(az)
    frames = []
    for x, y in places:
        sx, sy = x + sensor[0], y + sensor[1]
        with np.errstate(divide="ignore"):
            t = np.minimum(np.where(c > 0, (6.0 - sx) / c, (-6.0 - sx) / c), np.where(s > 0, (4.5 - sy) / s, (-4.5 - sy) / s))
        # the pillar: a disc of 0.5 m radius at (3, -1)
        px, py = 3.0 - sx, -1.0 - sy
        along, off = px * c + py * s, np.abs(px * s - py * c)
        hit = (along > 0) & (off < 0.5)
        t = np.where(hit, np.minimum(t, along - np.sqrt(np.maximum(0.25 - off * off, 0.0))), t)
        pts = np.stack([sensor[0] + t * c, sensor[1] + t * s, np.full(n, 0.5)], axis=1)
        frames.append((np.ascontiguousarray(pts), np.array([0.0, 0.0, 0.0, 1.0, x, y, 0.0]), sensor))
    return (0.1, -13.0, -10.0, 260, 200, 0.1, 1.5, 6.0), frames, places


def counts_of(occ):
    """counters whose readout at min_observations <= 100 is `occ`: (v, 100 - v) for v >= 0, (0, 0) for unknown"""
    occ = np.asarray(occ, dtype=np.int64)
    counts = np.zeros(occ.shape + (2,), dtype=np.uint16)
    known = occ >= 0
    counts[..., 0][known] = occ[known]
    counts[..., 1][known] = 100 - occ[known]
    return counts


def random_potential(shape, seed, unreached=0.2, levels=50):
    """uint32 potentials with many ties (few levels) and a share of unreached cells"""
    rng = np.random.default_rng(seed)
    pot = rng.integers(0, levels, shape).astype(np.uint32) * 3
    pot[rng.random(shape) < unreached] = NONE
    return pot
