"""numpy restatement of the grid's clearance and costmap (include/kicp.h, kicp_grid_clearance .. kicp_grid_last_window), written from
the header's text: the classes of a readout, the clearance by brute force over the list of source cells, the costmap rule, the
Nav2 cost table and the window of a frame.  Everything but the table is exact integer arithmetic: the tests compare with
np.array_equal.  Shared cases for the CPU and the GPU tests are at the end."""
import numpy as np

import grid_ref as gr


def classes(occ, occupied_thresh=0.65, unknown_is_obstacle=False):
    """-> (source, unknown-and-not-a-source) as bool arrays of occ's shape"""
    occ = np.asarray(occ, dtype=np.int8)
    source = occ.astype(np.float64) > occupied_thresh * 100.0
    unknown = occ < 0
    if unknown_is_obstacle:
        source = source | unknown
    return source, unknown & ~source


def clearance(occ, radius, occupied_thresh=0.65, unknown_is_obstacle=False, rect=None):
    """min dx^2 + dy^2 over ALL sources of the grid with dx^2 + dy^2 <= R^2, R^2 + 1 without one -> uint16 (h, w) of `rect`"""
    occ = np.asarray(occ, dtype=np.int8)
    H, W = occ.shape
    x0, y0, w, h = (0, 0, W, H) if rect is None else rect
    source, _ = classes(occ, occupied_thresh, unknown_is_obstacle)
    sy, sx = np.nonzero(source)
    far = radius * radius + 1
    yy, xx = np.mgrid[y0:y0 + h, x0:x0 + w]
    best = np.full(h * w, far, dtype=np.int64)
    cx, cy = xx.ravel().astype(np.int64), yy.ravel().astype(np.int64)
    for at in range(0, len(sx), 256):  # chunks of sources: cells x 256 distances at a time
        d2 = (cx[:, None] - sx[None, at:at + 256]) ** 2 + (cy[:, None] - sy[None, at:at + 256]) ** 2
        d2[d2 > radius * radius] = far
        best = np.minimum(best, d2.min(axis=1))
    return best.reshape(h, w).astype(np.uint16)


def clearance_by_offsets(occ, radius, occupied_thresh=0.65, unknown_is_obstacle=False):
    """The same brute force turned round, for grids with many sources: for every offset (dx, dy) with dx^2 + dy^2 <= R^2, from the
    farthest to the nearest, every cell that has a source at that offset takes dx^2 + dy^2 -> uint16, the full grid"""
    source, _ = classes(occ, occupied_thresh, unknown_is_obstacle)
    H, W = source.shape
    best = np.full((H, W), radius * radius + 1, dtype=np.uint16)
    offsets = [(dx * dx + dy * dy, dx, dy) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1) if dx * dx + dy * dy <= radius * radius]
    for d2, dx, dy in sorted(offsets, reverse=True):
        if abs(dx) >= W or abs(dy) >= H:
            continue
        # cells (x, y) with a source at (x + dx, y + dy)
        ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
        xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
        best[yd, xd][source[ys, xs]] = d2
    return best


def costmap(occ, table, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=False, rect=None, clear=None):
    """the costmap rule over `clear` (the clearance of the same arguments; computed when None) -> uint8 (h, w) of `rect`"""
    occ = np.asarray(occ, dtype=np.int8)
    table = np.asarray(table, dtype=np.uint8)
    radius = int(round(np.sqrt(len(table) - 2)))
    assert radius * radius + 2 == len(table)
    H, W = occ.shape
    x0, y0, w, h = (0, 0, W, H) if rect is None else rect
    if clear is None:
        clear = clearance(occ, radius, occupied_thresh, unknown_is_obstacle, rect)
    source, unknown = classes(occ, occupied_thresh, unknown_is_obstacle)
    source, unknown = source[y0:y0 + h, x0:x0 + w], unknown[y0:y0 + h, x0:x0 + w]
    t = table[clear].astype(np.int64)
    base = np.where(source, 254, np.where(unknown, 255, 0))
    takes = (t > 0) if inflate_unknown else (t >= 253)
    return np.where(base == 255, np.where(takes, t, 255), np.maximum(base, t)).astype(np.uint8)


def nav2_table(cell, radius, inscribed_radius, cost_scaling_factor):
    """-> (table uint8 [R^2 + 2], 252 * factor as float64 [R^2 + 2] - NaN where the entry is not computed from it)"""
    d2 = np.arange(radius * radius + 2, dtype=np.int64)
    d = np.sqrt(d2.astype(np.float64)) * cell
    raw = 252.0 * np.exp(-cost_scaling_factor * (d - inscribed_radius))
    table = np.where(d <= inscribed_radius, 253, np.floor(raw)).astype(np.uint8)
    raw[d <= inscribed_radius] = np.nan
    table[0], table[-1] = 254, 0
    raw[0] = raw[-1] = np.nan
    return table, raw


def window(cfg, pose, sensor_xyz):
    """(x0, y0, w, h): the (2 reach + 1)^2 cells around the sensor's cell clipped to the grid; zeros when none is inside"""
    _, _, (sx, sy) = gr.endpoints(cfg, np.zeros((0, 3)), pose, sensor_xyz)
    if not (np.isfinite(sx) and np.isfinite(sy)):
        return (0, 0, 0, 0)
    ax, bx = max(int(sx) - cfg["reach"], 0), min(int(sx) + cfg["reach"] + 1, cfg["width"])
    ay, by = max(int(sy) - cfg["reach"], 0), min(int(sy) + cfg["reach"] + 1, cfg["height"])
    return (ax, ay, bx - ax, by - ay) if ax < bx and ay < by else (0, 0, 0, 0)


def grown(rect, radius, width, height):
    """`rect` grown by `radius` cells on every side and clipped to the grid"""
    x0, y0, w, h = rect
    ax, ay = max(x0 - radius, 0), max(y0 - radius, 0)
    return (ax, ay, min(x0 + w + radius, width) - ax, min(y0 + h + radius, height) - ay)


# ---- the cases both test files run -----------------------------------------------------------------------------------------------
# a table with entries in each of {0, 1 .. 252, 253, 254}, for any radius: 254 on the source, 253 next to it, then decreasing, 0 from
# three quarters of the way out
def mixed_table(radius):
    d2 = np.arange(radius * radius + 2, dtype=np.int64)
    t = np.clip(252 - (d2 * 300) // max(radius * radius, 1), 0, 252)
    t[d2 * 4 > 3 * radius * radius] = 0
    t[0] = 254
    t[1:3] = 253
    t[-1] = 0
    return t.astype(np.uint8)


def pinned_8x6():
    """An 8 x 6 readout and its clearance at R = 3 (far = 10), written out cell by cell; row iy = 5 on top.  S source (100), u unknown
    (-1), . clear (0), f clear although busy (60 is not above 65):
        iy 5   . . . . . . . u          10 10 10 10 10 10  9 10
        iy 4   . . . . . . . .          10 10 10 10  8  5  4  5
        iy 3   . . f . . . . .          10  9 10 10  5  2  1  2
        iy 2   . . . . . . S .           5  4  5  8  4  1  0  1
        iy 1   . . . . . . . .           2  1  2  5  5  2  1  2
        iy 0   . S . . . . . .           1  0  1  4  8  5  4  5
    e.g. (3, 2): 2^2 + 2^2 = 8 from (1, 0) beats 3^2 = 9 from (6, 2); (3, 1) is 10 > 9 from (6, 2) and 5 from (1, 0); (6, 5) is exactly
    3 cells above (6, 2).  With unknown_is_obstacle the cell (7, 5) is a source as well, which changes the two top rows:
        iy 5                            10 10 10 10  9  4  1  0
        iy 4                            10 10 10 10  8  5  2  1"""
    occ = np.zeros((6, 8), dtype=np.int8)
    occ[0, 1], occ[2, 6], occ[3, 2], occ[5, 7] = 100, 100, 60, -1
    want = np.array([[1, 0, 1, 4, 8, 5, 4, 5], [2, 1, 2, 5, 5, 2, 1, 2], [5, 4, 5, 8, 4, 1, 0, 1], [10, 9, 10, 10, 5, 2, 1, 2], [10, 10, 10, 10, 8, 5, 4, 5],
                     [10, 10, 10, 10, 10, 10, 9, 10]], dtype=np.uint16)
    want_uio = want.copy()
    want_uio[4:] = [[10, 10, 10, 10, 8, 5, 2, 1], [10, 10, 10, 10, 9, 4, 1, 0]]
    return occ, 3, want, want_uio


def random_occupancy(width, height, source_fraction, seed, unknown_fraction=0.2):
    """a readout with about source_fraction cells at 100, unknown_fraction at -1, the rest spread over 0 .. 65 (never a source at 0.65)"""
    rng = np.random.default_rng(seed)
    occ = rng.integers(0, 66, (height, width)).astype(np.int8)
    u = rng.random((height, width))
    occ[u < unknown_fraction] = -1
    occ[u > 1.0 - source_fraction] = rng.integers(66, 101, int((u > 1.0 - source_fraction).sum())).astype(np.int8)
    return occ


def counts_of(occ):
    """counters whose readout at min_observations = 1 is `occ`: (v, 100 - v) for v >= 0, (0, 0) for unknown"""
    occ = np.asarray(occ, dtype=np.int64)
    counts = np.zeros(occ.shape + (2,), dtype=np.uint16)
    known = occ >= 0
    counts[..., 0][known] = occ[known]
    counts[..., 1][known] = 100 - occ[known]
    assert np.array_equal(gr.occupancy(counts), occ.astype(np.int8))
    return counts


def host_cases():
    """name -> (occ, radius): the cases of the issue's list, small enough for the brute force"""
    cases = {}
    occ, radius, _, _ = pinned_8x6()
    cases["pinned_8x6"] = (occ, radius)
    cases["one_cell_source"] = (np.array([[100]], dtype=np.int8), 2)
    cases["one_cell_clear"] = (np.array([[0]], dtype=np.int8), 2)
    cases["one_cell_unknown"] = (np.array([[-1]], dtype=np.int8), 2)
    none = random_occupancy(23, 17, 0.0, 3)
    cases["no_source"] = (none, 5)
    cases["all_sources"] = (np.full((9, 13), 100, dtype=np.int8), 4)
    corners = np.zeros((29, 37), dtype=np.int8)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 100
    corners[10:14, 15:20] = -1
    cases["corners_r20"] = (corners, 20)
    busy = random_occupancy(37, 29, 0.03, 11)
    for radius in (1, 3, 254):
        cases["random_37x29_r%d" % radius] = (busy, radius)
    return cases


def rectangles(width, height):
    """the full grid, single cells and rectangles touching each edge"""
    rects = [(0, 0, width, height), (width // 2, height // 2, 1, 1), (0, 0, 1, 1), (width - 1, height - 1, 1, 1)]
    if width >= 4 and height >= 4:
        rects += [(0, 1, 2, height - 2), (width - 3, 1, 3, 2), (1, 0, width - 2, 2), (2, height - 2, width - 3, 2)]
    return rects
