"""The case table of the frame-path regime tests, shared by tests/test_frame_cases.py (CPU: the premises of every case, from numpy and
the restatements alone, and the stand-alone host programs on the small ones) and tests/test_gpu_frame_regimes.py (GPU: kicp_grid.hpp
k_grid_mark, k_grid_rays, k_grid_apply and k_grid_readout; kicp_view.hpp k_view_render, k_view_classify, k_view_list and k_view_sweep).
Nothing here calls the GPU or the library: only numpy and grid_ref, grid_cases, view_ref, view_cases.  Seeded, deterministic, no files.

The constants restate the kernels' launch shapes as the cases were chosen for; the CPU test checks the cases against them, never the
library against them.  The `*_variant` functions are the restatements made wrong on purpose - a walk cut at 64 steps, a ray list cut
short, a plane word that belongs to one row, a corner cast without its range check, counters summed in 16 bits, a pixel without its
clamp, a conversion that flushes small floats, a sweep that makes one trip - so that the CPU test can show that each case's answer
depends on the regime it was built for.

Grid:  reach 4095 on 8191 x 9 and 9 x 8191 (two frames, the sensor moved); 524 588 points with more distinct endpoint cells than
k_grid_rays has waves; sensors whose window corner is 2^30, 2^30 + 1, beyond any int32 and the mirrored three; windows that are all
endpoints and all rays at reach 6 and 60; endpoint pairs in one plane word across two window rows; frames of 1 .. 257 points, every
lane a ray of its own; the readout at the counters' ends.
View:  res 8 and res 1024 (300 000 returns, directed clamp, tie and border points); window 3 and window 4 patches holding min_rays - 1
and min_rays returns, at corners, edges and inside; depths a float holds as +inf, as a denormal, as zero and as a rounding tie;
frames of 1 .. 257 points and 200 000 returns in one pixel; buckets of 63 .. 128 points losing all but the last, the last, the first
and nothing; a 3 x 3 x 3 block losing its centre, everything and one face; map points at exactly max_ray."""
import functools

import numpy as np

import grid_cases as gc
import grid_ref as gr
import view_cases as vc
import view_ref as vr


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


WAVE_EDGES = [1, 63, 64, 65, 255, 256, 257]  # around a wave and around a workgroup of a launch with one lane per point

# ---- grid --------------------------------------------------------------------------------------------------------------------------
GRID_BLOCK = 256      # lanes per workgroup of every grid kernel
GRID_RAY_GROUPS = 2048  # k_grid_rays is launched with min(blocks of the frame, 2048) workgroups
GRID_RAY_WAVES = GRID_RAY_GROUPS * (GRID_BLOCK // 64)  # 8 192: a ray list longer than this makes a wave stride
MAX_REACH = 4095
FAR_AWAY = -(1 << 30)  # kGridFarAway, and the last legal corner's mirror image


def grid_variant(cfg, counts, points, pose, sensor_xyz, max_steps=None, max_rays=None, word_rows=False, bare_cast=False):
    """gr.integrate over window indices as the kernels address them, made wrong on request: walks cut at `max_steps` steps, only the
    first `max_rays` distinct endpoint cells walked, every plane word decoded with the row of its first cell (`word_rows`), the
    window's corner cast to 32 bits without the range check (`bare_cast`).  With no request it IS gr.integrate (the CPU test holds it
    to that) -> (used, skipped, cells HIT, cells MISS)"""
    used, offs, (sx, sy) = gr.endpoints(cfg, points, pose, sensor_xyz)
    n_used = int(used.sum())
    if n_used == 0:
        return (0, len(used), 0, 0)
    W, H, reach = cfg["width"], cfg["height"], cfg["reach"]
    side = 2 * reach + 1

    def corner(s):
        c = int(s) - reach
        if bare_cast:
            return (c + 2 ** 31) % 2 ** 32 - 2 ** 31
        return c if -2 ** 30 <= c <= 2 ** 30 else FAR_AWAY

    gx0, gy0 = corner(sx), corner(sy)
    unique = np.unique(offs, axis=0)
    hit_at = (unique[:, 1] + reach) * side + unique[:, 0] + reach
    miss_at = [np.zeros(0, dtype=np.int64)]
    for dx, dy in unique[:max_rays]:
        ox, oy = gr.walk(dx, dy)
        miss_at.append(((oy + reach) * side + ox + reach)[:max_steps])
    planes = []
    for at in (hit_at, np.unique(np.concatenate(miss_at))):
        row = (at // 4 * 4) // side if word_rows else at // side
        col = at - row * side
        gx, gy = gx0 + col, gy0 + row
        ok = (col < side) & (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)
        plane = np.zeros((H, W), dtype=bool)
        plane[gy[ok], gx[ok]] = True
        planes.append(plane)
    hit, miss = planes[0], planes[1] & ~planes[0]
    for plane, which in ((hit, 0), (miss, 1)):
        c = counts[:, :, which]
        c[plane] = np.minimum(c[plane].astype(np.int64) + 1, 65535).astype(np.uint16)
    return (n_used, len(used) - n_used, int(hit.sum()), int(miss.sum()))


def run_variant(cfg, frames, **wrong):
    counts = np.zeros((cfg["height"], cfg["width"], 2), dtype=np.uint16)
    stats = [grid_variant(cfg, counts, pts, pose, sensor, **wrong) for pts, pose, sensor in frames]
    return counts, stats


def _at_cells(cfg, cells, z=0.0):
    """points 0.4 of a cell past the lower corner of the grid cells `cells` (int [n, 2], any integers)"""
    c = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
    return np.stack([cfg["origin_x"] + (c[:, 0] + 0.4) * cfg["cell"], cfg["origin_y"] + (c[:, 1] + 0.4) * cfg["cell"], np.full(len(c), z)], axis=1)


# 1. reach 4095
REACH_OFFSETS = [(4095, 0), (-4095, 0), (4095, 4095), (4095, -4095), (-4095, 4095), (-4095, -4095), (4095, 4094), (4096, 0)]  # the last one is out of reach


def reach_config(transposed):
    w, h = (9, 8191) if transposed else (8191, 9)
    return gr.make_config(0.25, 0.0, 0.0, w, h, -1.0, 1.0, 1023.75)


@functools.lru_cache(maxsize=None)
def reach_frames(transposed):
    """-> (cfg, two frames, the sensor's cell in each): the directed endpoints and 3 000 random returns out to 1 500 m, seen from the
    grid's middle cell and from a cell (+3, -2) from it"""
    cfg = reach_config(transposed)
    rng = np.random.default_rng(93)
    az, dist, z = rng.uniform(-np.pi, np.pi, 3000), rng.uniform(1.0, 1500.0, 3000), rng.uniform(-0.9, 0.9, 3000)
    frames, cells = [], []
    for shift in ((0, 0), (3, -2)):
        sx, sy = cfg["width"] // 2 + shift[0], cfg["height"] // 2 + shift[1]
        offs = np.array([(dy, dx) if transposed else (dx, dy) for dx, dy in REACH_OFFSETS])
        sensor = _at_cells(cfg, [(sx, sy)])[0]
        pts = np.concatenate([_at_cells(cfg, offs + (sx, sy)), np.stack([sensor[0] + dist * np.cos(az), sensor[1] + dist * np.sin(az), z], axis=1)])
        frames.append((frozen(np.ascontiguousarray(pts)), gc.IDENTITY, frozen(sensor)))
        cells.append((sx, sy))
    return cfg, frames, cells


# 2. more rays than k_grid_rays has waves
BIG_N = GRID_RAY_GROUPS * GRID_BLOCK + 300


@functools.lru_cache(maxsize=None)
def big_frame():
    """-> (cfg of gc.random_drive, (points, pose, sensor)): 524 588 points drawn as gc.random_drive draws its frames"""
    cfg, _ = gc.random_drive()
    rng = np.random.default_rng(94)
    n, sensor = BIG_N, np.array([0.2, 0.0, 0.4])
    pose = gc.tilted_pose(0.3, -0.2, rng.uniform(-np.pi, np.pi), np.deg2rad(rng.uniform(-4, 4)), np.deg2rad(rng.uniform(-4, 4)), z=rng.uniform(-0.05, 0.05))
    az, rng_m = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.2, 8.0, n)
    pts = np.stack([sensor[0] + rng_m * np.cos(az), sensor[1] + rng_m * np.sin(az), rng.uniform(-0.2, 2.0, n)], axis=1)
    pts[rng.integers(0, n, 3), rng.integers(0, 3, 3)] = [np.nan, np.inf, -np.inf]
    return cfg, (frozen(np.ascontiguousarray(pts)), frozen(pose), frozen(sensor))


@functools.lru_cache(maxsize=None)
def big_sequence():
    """-> (cfg, [the large frame, 65 points of another pose, the large frame again])"""
    cfg, big = big_frame()
    pts, pose, sensor = gc.random_drive()[1][1]
    return cfg, [big, (frozen(pts[:65].copy()), pose, sensor), big]


SPARSE_CFG = gr.make_config(0.1, -35.0, -35.0, 700, 700, 0.1, 1.5, 30.0)  # reach 300: a window of 601^2 cells inside the grid
SPARSE_CELLS = 9000


@functools.lru_cache(maxsize=None)
def sparse_big_frame():
    """The large frame above is dense: nearly every window cell is an endpoint, so its rays add next to nothing and a ray list cut short
    would not show.  This one has as many points in 9 000 distinct cells 200 .. 300 cells from the sensor, about 58 points each: the
    rays are long and few cross, so each of the 808 entries past the kernel's 8 192 waves carries MISS cells of its own"""
    rng = np.random.default_rng(102)
    cells = set()
    while len(cells) < SPARSE_CELLS:
        dx, dy = (int(v) for v in rng.integers(-300, 301, 2))
        if max(abs(dx), abs(dy)) >= 200:
            cells.add((dx, dy))
    cells = np.array(sorted(cells))[rng.permutation(SPARSE_CELLS)]
    which = np.concatenate([np.arange(SPARSE_CELLS), rng.integers(0, SPARSE_CELLS, BIG_N - SPARSE_CELLS)])[rng.permutation(BIG_N)]
    sensor = np.array([0.25, 0.05, 0.4])  # cell (352, 350)
    xy = SPARSE_CFG["origin_x"] + (np.array([352, 350]) + cells[which] + rng.uniform(0.1, 0.9, (BIG_N, 2))) * SPARSE_CFG["cell"]
    pts = np.concatenate([xy, rng.uniform(0.2, 1.4, (BIG_N, 1))], axis=1)
    return SPARSE_CFG, (frozen(np.ascontiguousarray(pts)), gc.IDENTITY, frozen(sensor))


# 3. a sensor no grid can be near
CFG16 = gr.make_config(0.25, -2.0, -2.0, 16, 16, -1.0, 1.0, 1.5)  # tests/test_gpu_grid.py's: reach 6


def far_sensors():
    """name -> (points, pose, sensor, the sensor's cell in x): two points one and two cells from the sensor, which are used; the
    window's corner is cell - 6.  The coordinates are exact in doubles (cells of 0.25 m; at 1e15 a double still resolves 0.125)"""
    out = {}
    cells = {"corner_2^30": 2 ** 30 + 6, "corner_2^30+1": 2 ** 30 + 7, "corner_-2^30": -2 ** 30 + 6, "corner_-2^30-1": -2 ** 30 + 5,
             "wraps_onto_the_grid": 2 ** 32 + 8}  # (the last one: a bare cast of its corner gives cell 2)
    for name, cell in cells.items():
        out[name] = (cell * 0.25 - 2.0 + 0.125, cell)
    out["x_1e15"], out["x_-1e15"] = (1.0e15, 4 * 10 ** 15 + 8), (-1.0e15, -4 * 10 ** 15 + 8)
    frames = {}
    for name, (x, cell) in out.items():
        sensor = np.array([x, 0.1, 0.0])
        pts = np.array([[x + 0.25, 0.1, 0.0], [x, 0.6, 0.2]])
        frames[name] = (pts, gc.IDENTITY, sensor, cell)
    return frames


# 4. all endpoints, all rays
CFG60 = gr.make_config(0.25, -16.0, -15.75, 128, 126, -1.0, 1.0, 15.0)  # reach 60; the window of the sensor below lies wholly inside
SENSOR60 = np.array([0.1, 0.1, 0.0])  # cell (64, 63): window cells 4 .. 124 and 3 .. 123
SENSOR16 = np.array([0.1, 0.1, 0.0])  # cell (8, 8) of CFG16: window cells 2 .. 14


def _window_case(reach):
    return (CFG16, SENSOR16, (8, 8)) if reach == 6 else (CFG60, SENSOR60, (64, 63))


def window_frame(reach, which, seed=95):
    """`which` = "endpoints": one point in every window cell; "rays": one in every cell of the ring at Chebyshev distance `reach`;
    shuffled -> (cfg, (points, pose, sensor))"""
    cfg, sensor, (sx, sy) = _window_case(reach)
    d = np.arange(-reach, reach + 1)
    dx, dy = (a.ravel() for a in np.meshgrid(d, d))
    if which == "rays":
        ring = np.maximum(np.abs(dx), np.abs(dy)) == reach
        dx, dy = dx[ring], dy[ring]
    order = np.random.default_rng(seed).permutation(len(dx))
    return cfg, (_at_cells(cfg, np.stack([sx + dx, sy + dy], axis=1)[order]), gc.IDENTITY, sensor)


# 5. plane words shared by two window rows
def shared_word_pairs():
    """[(window index of the first endpoint, ((dx, dy), (dx, dy)))] on CFG16 (side 13): the last cell of a window row and the first of
    the next, one pair per byte position 0 .. 3 of the first cell - the pair of position 3 does NOT share a word, for contrast"""
    reach, side = 6, 13
    out = []
    for row in range(4):
        at = (row + 1) * side - 1
        out.append((at, ((reach, row - reach), (-reach, row + 1 - reach))))
    return out


def offsets_frame(reach, offsets):
    cfg, sensor, (sx, sy) = _window_case(reach)
    return cfg, (_at_cells(cfg, np.asarray(offsets) + (sx, sy)), gc.IDENTITY, sensor)


# 6. frames that end inside a wave or a workgroup
def own_cell_frame(n, seed=96):
    """n points in n distinct cells of CFG60's window (never the sensor's own cell)"""
    d = np.arange(-60, 61)
    dx, dy = (a.ravel() for a in np.meshgrid(d, d))
    away = (dx != 0) | (dy != 0)
    pick = np.random.default_rng(seed + n).permutation(int(away.sum()))[:n]
    return offsets_frame(60, np.stack([dx[away][pick], dy[away][pick]], axis=1))


# 7. readout at the counters' ends
END_PAIRS = [(65535, 65535), (65535, 0), (0, 65535), (1, 65535), (65535, 1)]
MIN_OBSERVATIONS = [1, 65535, 131070, 131071, 2 ** 32 - 1]
READOUT_SHAPES = [(17, 15), (257, 1)]  # (width, height): 255 and 257 cells


def readout_counts(width, height, seed=97):
    """the end pairs, then random counters with a fifth of each side at 0 or 65535"""
    rng = np.random.default_rng(seed + width)
    c = rng.integers(0, 65536, (height * width, 2))
    ends = rng.random((height * width, 2))
    c[ends < 0.1], c[ends > 0.9] = 0, 65535
    c[:len(END_PAIRS)] = END_PAIRS
    c[-len(END_PAIRS):] = END_PAIRS[::-1]
    return c.astype(np.uint16).reshape(height, width, 2)


def occupancy_16bit_variant(counts, min_observations):
    """gr.occupancy with hits + misses summed in 16 bits"""
    c = np.asarray(counts, dtype=np.int64)
    hits, seen = c[..., 0], (c[..., 0] + c[..., 1]) % 65536
    out = np.full(seen.shape, -1, dtype=np.int8)
    known = (seen >= min_observations) & (seen > 0)
    out[known] = ((100 * hits[known] + seen[known] // 2) // seen[known]).astype(np.int8)
    return out


# ---- depth view ----------------------------------------------------------------------------------------------------------------------
VIEW_BLOCK = 256
AXES = {0: (0, 1, 2), 1: (0, 1, 2), 2: (1, 0, 2), 3: (1, 0, 2), 4: (2, 0, 1), 5: (2, 0, 1)}  # face -> (major axis, axis of a, axis of b)


def face_point(face, m, a, b):
    v = np.zeros(3)
    major, ia, ib = AXES[face]
    v[major], v[ia], v[ib] = (-m if face & 1 else m), a, b
    return v


def pixel_point(res, face, u, w, m, frac=0.5):
    """the offset at depth m through the pixel (u, w) of `face`, `frac` of a pixel past its lower border (exact for res a power of two)"""
    return face_point(face, m, m * ((u + frac) * 2.0 / res - 1.0), m * ((w + frac) * 2.0 / res - 1.0))


def view_case(cfg, frame, queries, pose=vc.IDENTITY, sensor=vc.ORIGIN):
    return dict(cfg=cfg, frame=np.ascontiguousarray(np.asarray(frame, dtype=np.float64).reshape(-1, 3)),
                queries=np.ascontiguousarray(np.asarray(queries, dtype=np.float64).reshape(-1, 3)), pose=np.asarray(pose, dtype=np.float64),
                sensor=np.asarray(sensor, dtype=np.float64))


def render_unclamped_variant(cfg, points, pose, sensor_xyz):
    """vr.render without the clamp of a pixel coordinate to res - 1: such a point writes where its index lands, in the next row or the
    next face, and nowhere when that is past the image"""
    res = cfg["res"]
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    c = vr.sensor_world(pose, sensor_xyz)
    depth = np.full(6 * res * res, np.inf, dtype=np.float32)
    v = vr.transform(pose, p) - c
    with np.errstate(all="ignore"):
        ok, m, face, _, _ = vr.project(cfg, v)
        major = face // 2
        a = np.where(major == 0, v[:, 1], v[:, 0])
        b = np.where(major == 2, v[:, 1], v[:, 2])
        u, w = np.floor((a / m + 1.0) * (res / 2.0)), np.floor((b / m + 1.0) * (res / 2.0))
    ok &= np.all(np.isfinite(p), axis=1)
    at = ((face * res + np.where(ok, w, 0).astype(np.int64)) * res + np.where(ok, u, 0).astype(np.int64))
    ok &= at < depth.size
    with np.errstate(over="ignore"):
        np.minimum.at(depth, at[ok], m[ok].astype(np.float32))
    return depth.reshape(6, res, res)


def flushed_variant(depth):
    """the image a conversion that flushes denormal floats to zero would leave"""
    out = depth.copy()
    out[np.abs(out) < np.finfo(np.float32).tiny] = 0.0
    return out


# 8. the smallest and the largest image
@functools.lru_cache(maxsize=None)
def res8_case():
    rng = np.random.default_rng(98)
    cfg = vr.make_config(8, 0, 1, 10.0, 0.1, 0.01)
    frame = rng.normal(size=(300, 3))
    frame *= (rng.uniform(3.0, 12.0, 300) / np.abs(frame).max(axis=1))[:, None]
    corners = [face_point(f, 6.0, sa * 6.0, sb * 6.0) for f in (0, 1) for sa in (-1, 1) for sb in (-1, 1)]
    pose = np.concatenate([vc._unit([0.02, -0.03, 0.5, 0.86]), [1.5, -0.5, 0.25]])
    case = view_case(cfg, frame, rng.uniform(-11, 11, (500, 3)) + pose[4:], pose=pose, sensor=np.array([0.1, 0.0, 0.3]))
    exact = view_case(cfg, np.array(corners), 0.5 * np.array(corners))  # identity pose: a / m == +-1 exactly on the x faces
    return case, exact


RES1024 = vr.make_config(1024, 4, 81, 40.0, 0.05, 0.01)
PATCH = (200, 264)  # pixels of face 0, both ways, that a dense patch at m = 30 fills: only there can all 81 pixels of a window hold a return


def directed_1024():
    """[(offset, expected (face, u, w))]: m = 8 under the identity pose.  below(8) / 8 + 1 rounds to 2.0, so the pixel coordinate
    1024 is clamped on every face; -below(8) / 8 + 1 = 2^-53 lands in pixel 0; a / m = +-1 exactly exists on the x faces only (a tie
    goes to x); the three tie rules; a / m = 100 / 512 exactly on a border (the upper pixel's) and 2^-40 below it"""
    below = np.nextafter(8.0, 0.0)
    out = []
    for face in range(6):
        for sa in (-1, 1):
            for sb in (-1, 1):
                out.append((face_point(face, 8.0, sa * below, sb * below), (face, 1023 if sa > 0 else 0, 1023 if sb > 0 else 0)))
    for face in (0, 1):
        for sa in (-1, 1):
            for sb in (-1, 1):
                out.append((face_point(face, 8.0, sa * 8.0, sb * 8.0), (face, 1023 if sa > 0 else 0, 1023 if sb > 0 else 0)))
    out.append((np.array([3.0, 3.0, 1.0]), (0, 1023, 682)))     # |x| == |y|: x
    out.append((np.array([1.0, 4.0, -4.0]), (2, 640, 0)))       # |y| == |z|: y
    out.append((np.array([-5.0, 2.0, -5.0]), (1, 716, 0)))      # |x| == |z|: x
    out.append((np.array([-2.0, 2.0, 2.0]), (1, 1023, 1023)))   # all three: x
    out.append((np.array([8.0, 100.0 / 64.0, -37.0 / 64.0]), (0, 612, 475)))
    out.append((np.array([8.0, 100.0 / 64.0 - 2.0 ** -37, -37.0 / 64.0 - 2.0 ** -37]), (0, 611, 474)))  # (a step that survives the + 1.0)
    return out


@functools.lru_cache(maxsize=None)
def res1024_case():
    """300 000 random returns from 5 m to beyond max_ray, the dense patch, the directed points; 20 000 queries: random ones, 2 000 in
    front of and behind the patch, and the directed points at half and at one and a half times their depth"""
    rng = np.random.default_rng(99)
    frame = rng.normal(size=(300000, 3))
    frame *= (rng.uniform(5.0, 52.0, 300000) / np.abs(frame).max(axis=1))[:, None]
    g = np.arange(PATCH[0], PATCH[1])
    u, w = (a.ravel() for a in np.meshgrid(g, g))
    patch = np.array([pixel_point(1024, 0, a, b, 30.0) for a, b in zip(u, w)])
    directed = np.array([v for v, _ in directed_1024()])
    near = np.array([pixel_point(1024, 0, a, b, m, f) for a, b, m, f in zip(rng.integers(PATCH[0] - 6, PATCH[1] + 6, 2000), rng.integers(PATCH[0] - 6, PATCH[1] + 6, 2000),
                                                                            rng.uniform(2.0, 39.0, 2000), rng.uniform(0.05, 0.95, 2000))])
    queries = np.concatenate([rng.uniform(-45, 45, (20000 - 2000 - 2 * len(directed), 3)), near, 0.5 * directed, 1.5 * directed])
    case = view_case(RES1024, np.concatenate([frame, patch, directed]), queries)
    frozen(case["frame"], case["queries"])
    return case


# 9. window 3, and the fullest window
def window_pixels(res, window, u, w):
    """the pixels of the window round (u, w) that lie on the face, outermost ring first"""
    px = [(i, j) for j in range(w - window, w + window + 1) for i in range(u - window, u + window + 1) if 0 <= i < res and 0 <= j < res]
    return sorted(px, key=lambda p: (-max(abs(p[0] - u), abs(p[1] - w)), p[1], p[0]))


def patch_places(res, window):
    """name -> the query's pixel: the four corners, the middle of the four edges, the middle of the face - the middle alone where the
    windows of the others would overlap (window 4 at res 16)"""
    last, mid = res - 1, res // 2
    if 2 * window >= mid:
        return {"inside": (mid, mid)}
    return {"corner_00": (0, 0), "corner_10": (last, 0), "corner_01": (0, last), "corner_11": (last, last), "edge_left": (0, mid), "edge_right": (last, mid),
            "edge_low": (mid, 0), "edge_high": (mid, last), "inside": (mid, mid)}


def patch_case(res, window, min_rays, filled, face=0):
    """One frame and one query per place of patch_places(res, window) - the patches do not overlap: the first `filled` pixels of the query's
    clipped window (outermost ring first, so a smaller window sees fewer) hold a return at m = 8, the query sits at m = 4 in the middle
    of its pixel.  -> (case, expected verdicts: seen through iff min(filled, pixels on the face) >= min_rays)"""
    cfg = vr.make_config(res, window, min_rays, 10.0, 0.25, 0.0)
    frame, queries, want = [], [], []
    for name, (u, w) in patch_places(res, window).items():
        px = window_pixels(res, window, u, w)
        frame += [pixel_point(res, face, i, j, 8.0) for i, j in px[:filled]]
        queries.append(pixel_point(res, face, u, w, 4.0))
        want.append(vc.T if min(filled, len(px)) >= min_rays else vc.K)
    return view_case(cfg, np.array(frame).reshape(-1, 3), np.array(queries)), want


def patch_cases():
    """[(id, res, window, min_rays, filled)]: window 3 with min_rays 1, 25 and 49, window 4 with 81, each at min_rays - 1 and min_rays"""
    out = []
    for res in (16, 64):
        for window, min_rays in ((3, 1), (3, 25), (3, 49), (4, 81)):
            for filled in (min_rays - 1, min_rays):
                out.append(("res%d_w%d_min%d_filled%d" % (res, window, min_rays, filled), res, window, min_rays, filled))
    return out


# 10. depths a float cannot hold as a normal number
TINY_CFG = vr.make_config(16, 0, 1, 1.0e39, 0.0, 0.0)
F32 = np.float32


def tiny_case():
    """Five returns along five axes, each alone in pixel (8, 8) of its face, and queries before and behind the float each leaves:
      +x  5e38          (float) is +inf: used, the pixel stays empty, every query is kept
      -x  1e-40         a denormal float D: a query at D is kept, one ulp of a double nearer is seen through
      +y  3e-46         rounds to 0.0f: a finite pixel nothing can lie in front of
      -y  1 + 2^-24     a tie, to even: 1.0f - a query at 1.0 is kept, one at 1 - 2^-53 seen through
      +z  1 + 3 2^-24   a tie, to even: 1 + 2^-22 - a query at the return's own depth is seen through, one at 1 + 2^-22 kept
    -> (case, expected verdicts, expected finite pixels {(face, w, u): float32})"""
    d40 = float(F32(1.0e-40))
    returns = [(0, 5.0e38), (1, 1.0e-40), (2, 3.0e-46), (3, 1.0 + 2.0 ** -24), (4, 1.0 + 3 * 2.0 ** -24)]
    queries = [(0, 4.0e38, vc.K), (0, 1.0e30, vc.K), (1, d40, vc.K), (1, np.nextafter(d40, 0.0), vc.T), (1, 1.0e-40, vc.K), (1, 5.0e-41, vc.T), (1, 2.0e-40, vc.K),
               (2, 1.0e-46, vc.K), (2, 3.0e-46, vc.K), (2, 5.0e-324, vc.K), (3, 1.0, vc.K), (3, np.nextafter(1.0, 0.0), vc.T), (3, 1.0 + 2.0 ** -25, vc.K),
               (3, 1.0 + 2.0 ** -24, vc.K), (4, 1.0 + 3 * 2.0 ** -24, vc.T), (4, 1.0 + 2.0 ** -22, vc.K), (4, np.nextafter(1.0 + 2.0 ** -22, 0.0), vc.T),
               (4, 1.0 + 2.0 ** -23, vc.T)]
    case = view_case(TINY_CFG, np.array([face_point(f, m, 0.0, 0.0) for f, m in returns]), np.array([face_point(f, m, 0.0, 0.0) for f, m, _ in queries]))
    pixels = {(1, 8, 8): F32(1.0e-40), (2, 8, 8): F32(0.0), (3, 8, 8): F32(1.0), (4, 8, 8): F32(1.0 + 2.0 ** -22)}
    return case, [v for _, _, v in queries], pixels


# 11. counts at the wave and workgroup edges; one contended pixel
@functools.lru_cache(maxsize=None)
def edge_points():
    """-> (cfg, pose, sensor, 257 frame points, 70 000 world queries): random directions, depths from 3 m to beyond max_ray"""
    rng = np.random.default_rng(100)
    cfg = vr.make_config(32, 1, 2, 8.0, 0.1, 0.02)
    pose = np.concatenate([vc._unit([0.03, -0.05, 0.6, 0.8]), [2.5, -1.25, 0.3]])
    frame = rng.normal(size=(257, 3))
    frame *= (rng.uniform(3.0, 9.5, 257) / np.abs(frame).max(axis=1))[:, None]
    return cfg, pose, np.array([0.2, 0.0, 0.5]), frozen(frame), frozen(rng.uniform(-9, 9, (70000, 3)) + pose[4:])


CONTENDED_N = 200000
CONTENDED_MIN = 2.5


def contended_frame(minimum_first):
    """200 000 returns in the pixel (8, 8) of face 0 at res 16: depths 3 .. 9 m, and the known minimum first or last"""
    d = np.random.default_rng(101).uniform(3.0, 9.0, CONTENDED_N)
    d[0 if minimum_first else -1] = CONTENDED_MIN
    return d[:, None] * np.array([1.0, 0.05, 0.05])


# 12. bucket lengths at the sweep's trip edges
CAP128 = 128
BUCKET_LENGTHS = [63, 64, 65, 127, 128]
BUCKET_PATTERNS = ["all_but_last", "only_last", "only_first", "none"]
GONE_LAYERS, KEPT_LAYERS = (10.005, 10.095), (10.3, 10.42)  # behind vc.wall() under vc.WALL_CFG: x < 10.098 is seen through


def bucket128(pattern, j, k):
    """one voxel (10, j, k) at max_points_per_voxel 128, point i seen through where pattern[i], in insertion order.  A layer holds 121
    points 0.091 m apart; the second layer of a kind is shifted by half a step and lies 0.09 m (0.12 m) behind the first, so no two
    points of the voxel are nearer than the map's resolution 1 / sqrt(128) = 0.0884 m"""
    lat = vc.lattice(CAP128)
    half = 0.5 * 1.03 / np.sqrt(CAP128)
    used = {True: 0, False: 0}
    pts = []
    for gone in pattern:
        n = used[bool(gone)]
        used[bool(gone)] = n + 1
        layer, at = divmod(n, len(lat))
        x = (GONE_LAYERS if gone else KEPT_LAYERS)[layer]
        pts.append([x, j + lat[at, 0] + layer * half, k + lat[at, 1] + layer * half])
    return np.array(pts)


def bucket_pattern(name, n):
    p = np.zeros(n, dtype=bool)
    if name == "all_but_last":
        p[:-1] = True
    elif name == "only_last":
        p[-1] = True
    elif name == "only_first":
        p[0] = True
    return p


def bucket_sweep_cases():
    """name -> dict(vs, cap, points, pattern) as vc.sweep_cases(): per pattern five voxels (10, j, 0) and (10, j, -1), one per length"""
    places = [(-2, 0), (-1, 0), (0, 0), (1, 0), (-1, -1)]
    cases = {}
    for name in BUCKET_PATTERNS:
        patterns = [bucket_pattern(name, n) for n in BUCKET_LENGTHS]
        cases[name] = dict(vs=1.0, cap=CAP128, points=np.concatenate([bucket128(p, j, k) for p, (j, k) in zip(patterns, places)]), pattern=np.concatenate(patterns))
    return cases


def one_trip_variant(cfg, depth, c, cloud, vs):
    """vr.sweep's keep mask when only the first 64 points of every bucket are judged (`cloud` bucket-sorted)"""
    keep, _ = vr.sweep(cfg, depth, c, cloud, vs)
    key = np.floor(np.asarray(cloud) / vs)
    new = np.concatenate([[True], np.any(key[1:] != key[:-1], axis=1)])
    start = np.maximum.accumulate(np.where(new, np.arange(len(cloud)), 0))
    return keep | (np.arange(len(cloud)) - start >= 64)


# 13. erased voxels and their 26 neighbours
ONE_PIXEL_CFG = vr.make_config(64, 0, 1, 30.0, 0.2, 0.02)  # window 0: a return sees through its own pixel only


def block_cases():
    """name -> dict(vs, cap, points, cfg, frame, erased): a 3 x 3 x 3 block of voxels of 1 m, three or four points each.
      centre  voxels 9 .. 11 in x.  The frame fills ONLY the pixel (32, 32) of face 0 (0 <= y / x, z / x < 1 / 32) at x = 10.5; the centre
              voxel (10, 0, 0) keeps its four points inside that pixel at x = 10.02, every other voxel keeps its points at y, z offsets
              of 0.45 and more - another pixel - so only the centre loses everything
      all     voxels 7 .. 9 in x behind vc.wall(): everything is seen through, 27 voxels erase each other concurrently
      face    voxels 9 .. 11 in x behind vc.wall(): the face x = 9 goes (x = 9.5 < 10.098), the points at x = 10.5 and 11.5 stay"""
    def block(x0, centre=None):
        pts = []
        for i in range(3):
            for j in (-1, 0, 1):
                for k in (-1, 0, 1):
                    if centre is not None and (i, j, k) == (1, 0, 0):
                        pts += [[x0 + 1.02, y, z] for y in (0.03, 0.28) for z in (0.03, 0.28)]
                    else:
                        pts += [[x0 + i + 0.5, j + 0.45 + 0.25 * t, k + 0.5 + 0.2 * (t % 2)] for t in range(3)]
        return np.array(pts)

    own = np.array([[10.5, y, z] for y in (0.05, 0.15, 0.25) for z in (0.05, 0.15, 0.25)])
    return {"centre": dict(vs=1.0, cap=20, points=block(9.0, centre=True), cfg=ONE_PIXEL_CFG, frame=own, erased=1),
            "all": dict(vs=1.0, cap=20, points=block(7.0), cfg=vc.WALL_CFG, frame=vc.wall(), erased=27),
            "face": dict(vs=1.0, cap=20, points=block(9.0), cfg=vc.WALL_CFG, frame=vc.wall(), erased=9)}


# 14. the range cull and a view that sees nothing
CULL_CFG = vr.make_config(16, 0, 1, 10.0, 0.1, 0.0)
CULL_SENSOR = np.array([0.375, -0.125, 0.25])  # exact in binary, off the lattice of 1 m and of 0.3 m voxels


def cull_case():
    """-> dict(points, frame, at_max_ray (mask), beyond (mask)): per face one map point at EXACTLY max_ray = 10 from the sensor (in range:
    counted and, nothing being returned there, kept) and one an ulp beyond; a wall of returns at 9 m on +x with map points at 5 m in front
    of it (removed); and a point 13 m out, whose voxel's box lies wholly beyond max_ray at 1 m and at 0.3 m voxels"""
    c = CULL_SENSOR
    at, beyond = [], []
    for face in range(6):
        at.append(c + face_point(face, 10.0, 0.6, -0.4))
        beyond.append(c + face_point(face, 10.0 + 2.0 ** -40, -0.7, 0.3))  # (exact after adding c, whose parts are eighths)
    g = np.arange(-8, 9) * 0.25
    y, z = np.meshgrid(g, g, indexing="ij")
    frame = np.stack([np.full(y.size, 9.0), y.ravel(), z.ravel()], axis=1) + c
    front = np.array([[5.0, 0.2, 0.3], [5.0, -0.9, 0.4], [5.2, 0.5, -1.1]]) + c
    far = np.array([[13.0, 0.1, 0.1]]) + c
    points = np.concatenate([np.array(at), np.array(beyond), front, far])
    mask = np.zeros(len(points), dtype=bool)
    at_mask, beyond_mask, far_mask = mask.copy(), mask.copy(), mask.copy()
    at_mask[:6], beyond_mask[6:12], far_mask[-1] = True, True, True
    return dict(points=points, frame=frame, at_max_ray=at_mask, beyond=beyond_mask, far=far_mask, removed=3)


NAN_POSE = np.array([0.0, 0.0, 0.0, 1.0, np.nan, 0.0, 0.0])
