"""Restatement of the cost-to-go field over a costmap and of the path down it (include/kicp.h, kicp_plan_weights .. kicp_grid_potential),
written from the header's text, in two independent ways that must agree: a heap Dijkstra over Python integers that clamps at the end,
and vectorised numpy min-plus sweeps of the clamped recurrence to its fixed point.  Also the path rule and the weights rule.  Everything
is exact integer arithmetic: the tests compare with np.array_equal.  Shared cases for the CPU and the GPU tests are at the end."""
import heapq

import numpy as np

UNREACHED = 0xFFFFFFFF
MAX_POTENTIAL = 0xFFFFFFFE
# the neighbours in the path's order: +x, -x, +y, -y, (+x, +y), (-x, +y), (+x, -y), (-x, -y)
NEIGHBOURS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]


def edge(qu, qv, diagonal):
    s = qu + qv
    return (181 * s + 64) >> 7 if diagonal else s


def weights(neutral=50, factor_num=4, factor_den=5, lethal_from=253, unknown_weight=0):
    w = np.zeros(256, dtype=np.uint8)
    for b in range(255):
        if b < lethal_from:
            w[b] = min(255, neutral + b * factor_num // factor_den)
    w[255] = unknown_weight
    return w


def _q(costmap, weight):
    return np.asarray(weight, dtype=np.uint8)[np.asarray(costmap, dtype=np.uint8)].astype(np.int64)


def stats_of(pot, q, goals, max_potential):
    """(goals used, cells below max_potential, cells equal to it)"""
    return (sum(1 for x, y in goals if q[y, x] > 0), int((pot < max_potential).sum()), int((pot == max_potential).sum()))


def potential_dijkstra(costmap, weight, goals, max_potential=MAX_POTENTIAL):
    """-> (uint32 (H, W), stats): least sums of edge weights by a heap Dijkstra over Python integers, clamped at the end"""
    q = _q(costmap, weight)
    H, W = q.shape
    ql = q.tolist()
    dist = [[None] * W for _ in range(H)]
    heap = []
    for x, y in goals:
        assert 0 <= x < W and 0 <= y < H
        if ql[y][x] > 0 and dist[y][x] is None:
            dist[y][x] = 0
            heap.append((0, x, y))
    heapq.heapify(heap)
    while heap:
        d, x, y = heapq.heappop(heap)
        if d != dist[y][x]:
            continue
        for k, (dx, dy) in enumerate(NEIGHBOURS):
            nx, ny = x + dx, y + dy
            if not (0 <= nx < W and 0 <= ny < H) or ql[ny][nx] == 0:
                continue
            nd = d + edge(ql[y][x], ql[ny][nx], k >= 4)
            if dist[ny][nx] is None or nd < dist[ny][nx]:
                dist[ny][nx] = nd
                heapq.heappush(heap, (nd, nx, ny))
    pot = np.array([[UNREACHED if d is None else min(d, max_potential) for d in row] for row in dist], dtype=np.uint32)
    return pot, stats_of(pot, q, goals, max_potential)


def potential_sweeps(costmap, weight, goals, max_potential=MAX_POTENTIAL):
    """-> (uint32 (H, W), stats, sweeps): the clamped recurrence pot(c) = min(pot(c), min(pot(n) + edge(c, n), max_potential)) swept
    over the whole grid at once, from every neighbour direction, until nothing changes"""
    q = _q(costmap, weight)
    H, W = q.shape
    big = np.int64(1) << 62
    Q = np.zeros((H + 2, W + 2), dtype=np.int64)
    Q[1:-1, 1:-1] = q
    P = np.full((H + 2, W + 2), big, dtype=np.int64)
    for x, y in goals:
        if q[y, x] > 0:
            P[y + 1, x + 1] = 0
    passable = q > 0
    sweeps = 0
    while True:
        sweeps += 1
        best = P[1:-1, 1:-1].copy()
        for k, (dx, dy) in enumerate(NEIGHBOURS):
            Pn, Qn = P[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx], Q[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
            s = q + Qn
            e = ((181 * s + 64) >> 7) if k >= 4 else s
            cand = np.where((Qn > 0) & (Pn < big), np.minimum(Pn + e, max_potential), big)
            best = np.minimum(best, cand)
        best = np.where(passable, best, big)
        if np.array_equal(best, P[1:-1, 1:-1]):
            break
        P[1:-1, 1:-1] = best
    pot = np.where(P[1:-1, 1:-1] >= big, UNREACHED, P[1:-1, 1:-1]).astype(np.uint32)
    return pot, stats_of(pot, q, goals, max_potential), sweeps


def path(pot, costmap, weight, start):
    """-> list of (x, y), or "unreachable" / "clamped" """
    q = _q(costmap, weight)
    H, W = q.shape
    x, y = start
    if int(pot[y, x]) == UNREACHED:
        return "unreachable"
    cells = [(x, y)]
    while int(pot[y, x]) != 0:
        for k, (dx, dy) in enumerate(NEIGHBOURS):
            nx, ny = x + dx, y + dy
            if 0 <= nx < W and 0 <= ny < H and q[ny, nx] > 0 and int(pot[ny, nx]) != UNREACHED and \
                    int(pot[y, x]) == int(pot[ny, nx]) + edge(int(q[y, x]), int(q[ny, nx]), k >= 4):
                x, y = nx, ny
                break
        else:
            return "clamped"
        cells.append((x, y))
    return cells


# ---- the cases the test files run --------------------------------------------------------------------------------------------------
IDENTITY = np.arange(256, dtype=np.uint8)  # q = the costmap's byte itself: 0 impassable


def pinned_8x6():
    """An 8 x 6 costmap, weights, one goal at (0, 0) and its potential written out cell by cell; row y = 5 on top.  `.` q = 1, `W`
    impassable, `5` q = 5.  An orthogonal step between two `.` weighs 2, a diagonal one (181 * 2 + 64) >> 7 = 3; into or out of the
    `5` they weigh 6 and (181 * 6 + 64) >> 7 = 8.
        y 5   . . . . . . . .          10 11 12 13 15 17 19 21
        y 4   . . . . . . . .           8  9 10 12 14 16 18 20
        y 3   . . . 5 . . . .           6  7  9 15 15 17 19 18
        y 2   . W W W W W W .           4  -  -  -  -  -  - 16
        y 1   . . . . . . . .           2  3  5  7  9 11 13 15
        y 0   G . . . . . . .           0  2  4  6  8 10 12 14
    e.g. (7, 2) is reached round the wall's end from (6, 1): 13 + 3; (3, 3) only through its expensive edges: 9 + 6 from (2, 3);
    (4, 3) avoids it: (3, 4) + 3 = 15, and (7, 3) = 18 comes down the right-hand side while (6, 3) = 19 is the one cell three ways
    reach at the same sum.  With max_potential = 17 the six cells above 17 read 17 and the two at 17 keep it: 8 cells equal, 34 below."""
    costmap = np.zeros((6, 8), dtype=np.uint8)
    costmap[2, 1:7] = 254
    costmap[3, 3] = 100
    weight = np.zeros(256, dtype=np.uint8)
    weight[0], weight[100] = 1, 5
    U = UNREACHED
    want = np.array([[0, 2, 4, 6, 8, 10, 12, 14], [2, 3, 5, 7, 9, 11, 13, 15], [4, U, U, U, U, U, U, 16], [6, 7, 9, 15, 15, 17, 19, 18],
                     [8, 9, 10, 12, 14, 16, 18, 20], [10, 11, 12, 13, 15, 17, 19, 21]], dtype=np.uint32)
    return costmap, weight, [(0, 0)], want


def random_costmap(width, height, seed, impassable=0.3):
    """bytes 1 .. 255 with about `impassable` of the cells 0; with IDENTITY weights q is the byte"""
    rng = np.random.default_rng(seed)
    cm = rng.integers(1, 256, (height, width)).astype(np.uint8)
    cm[rng.random((height, width)) < impassable] = 0
    return cm


def serpentine(width=130, height=100):
    """a wall on every fourth row with its gap at alternating ends: the one path from the top to the bottom runs the grid's width
    once per four rows and crosses tile borders about a hundred times"""
    cm = np.full((height, width), 1, dtype=np.uint8)
    for k, y in enumerate(range(3, height, 4)):
        cm[y, :] = 0
        cm[y, (width - 1) if k % 2 == 0 else 0] = 1
    return cm


def enclosed(width=40, height=36):
    """a closed ring of impassable cells around a region that no goal outside reaches"""
    cm = np.full((height, width), 7, dtype=np.uint8)
    cm[10, 12:25] = cm[22, 12:25] = 0
    cm[10:23, 12] = cm[10:23, 24] = 0
    return cm


def small_cases():
    """name -> (costmap, weight, goals, max_potential): small enough for both restatements"""
    cases = {}
    cm, weight, goals, _ = pinned_8x6()
    cases["pinned_8x6"] = (cm, weight, goals, MAX_POTENTIAL)
    cases["pinned_8x6_clamped"] = (cm, weight, goals, 17)
    cases["one_cell"] = (np.array([[9]], dtype=np.uint8), IDENTITY, [(0, 0)], MAX_POTENTIAL)
    cases["column_1x70"] = (random_costmap(1, 70, 5, 0.05), IDENTITY, [(0, 69)], MAX_POTENTIAL)
    cases["row_70x1"] = (random_costmap(70, 1, 6, 0.05), IDENTITY, [(0, 0), (69, 0)], MAX_POTENTIAL)
    rnd = random_costmap(96, 70, 1)
    rnd[3, 4] = rnd[60, 90] = 200
    cases["random_96x70"] = (rnd, IDENTITY, [(4, 3), (90, 60)], MAX_POTENTIAL)
    cases["random_96x70_clamped"] = (rnd, IDENTITY, [(4, 3), (90, 60)], 5000)
    cases["random_96x70_clamp_1"] = (rnd, IDENTITY, [(4, 3)], 1)
    ring = enclosed()
    cases["enclosed"] = (ring, IDENTITY, [(2, 2)], MAX_POTENTIAL)
    cases["enclosed_goal_inside"] = (ring, IDENTITY, [(18, 16)], MAX_POTENTIAL)
    cases["goal_impassable_alone"] = (ring, IDENTITY, [(12, 15)], MAX_POTENTIAL)
    cases["goal_impassable_beside_a_good_one"] = (ring, IDENTITY, [(12, 15), (30, 30), (24, 11)], MAX_POTENTIAL)
    nav = random_costmap(50, 45, 9, 0.0)
    nav[nav > 252] = 252
    nav[np.random.default_rng(2).random(nav.shape) < 0.2] = 254
    nav[np.random.default_rng(3).random(nav.shape) < 0.1] = 255
    nav[0, 0] = 0
    cases["nav2_weights"] = (nav, weights(), [(0, 0)], MAX_POTENTIAL)
    cases["nav2_weights_through_unknown"] = (nav, weights(unknown_weight=255), [(0, 0), (0, 0)], MAX_POTENTIAL)
    for w, h in ((31, 33), (32, 32), (33, 31), (63, 65), (64, 64), (65, 63)):
        cm = random_costmap(w, h, w * 100 + h, 0.15)
        cm[0, 0] = cm[0, w - 1] = cm[h - 1, 0] = cm[h - 1, w - 1] = 3
        cases["corners_%dx%d" % (w, h)] = (cm, IDENTITY, [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)], MAX_POTENTIAL)
    across = np.full((65, 65), 2, dtype=np.uint8)
    for dx, dy in NEIGHBOURS:  # (31, 31) reaches the goal (32, 32) by the diagonal step only, across four tiles
        if (dx, dy) != (1, 1):
            across[31 + dy, 31 + dx] = 0
    cases["diagonal_across_four_tiles"] = (across, IDENTITY, [(32, 32)], MAX_POTENTIAL)
    corner = random_costmap(65, 65, 8, 0.1)
    corner[31, 31] = corner[32, 32] = 5
    cases["goal_on_a_tile_corner_65x65"] = (corner, IDENTITY, [(31, 31)], MAX_POTENTIAL)
    return cases
