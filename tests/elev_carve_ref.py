"""numpy and Python-integer restatement of the height columns' carve (include/kicp.h, CARVING ALONG THE FRAME'S RAYS), written from
the header's text on top of tests/elev_ref.py: which points carve, the set of triples, the cell and the mask of every step of every
ray, the carved columns and the nine statistics of an update.  Everything is exact: the tests compare with np.array_equal.

Indices are int64 arrays (every product stays below 2^29); a step's mask is formed from two shifts by 0 .. 63 of a full word, with the
empty cases set to zero by comparison, and step_mask() states the same in Python integers, where no shift can go wrong; the columns are
Python integers where they are carved."""
import numpy as np

import elev_ref as er
import grid_ref as gr

U64 = np.uint64
FULL = (1 << 64) - 1
S_MIN, S_MAX = -32768, 32767


def sensor(cfg, pose, sensor_xyz):
    """-> (sx, sy, ss): the sensor's cell (floats, not finite when the pose or the origin is not) and its slab, None when out of range"""
    r0, r1, t0, t1 = gr.pose_to_rt(pose)
    r2, t2 = er.row2(pose)
    with np.errstate(all="ignore"):
        sen = np.asarray(sensor_xyz, dtype=np.float64).reshape(3)
        sx = gr._cell(np.float64(gr._world(r0, t0, sen[0], sen[1], sen[2])), cfg["origin_x"], cfg["cell"])
        sy = gr._cell(np.float64(gr._world(r1, t1, sen[0], sen[1], sen[2])), cfg["origin_y"], cfg["cell"])
        ss = np.floor((np.float64(gr._world(r2, t2, sen[0], sen[1], sen[2])) - cfg["z_origin"]) / cfg["slab"])
    return sx, sy, (int(ss) if S_MIN <= ss <= S_MAX else None)  # (a NaN fails the comparison)


def triples(cfg, points, pose, sensor_xyz):
    """-> (carve_points, sorted list of the distinct (dx, dy, es) of the eligible points, ss); nothing when ss is out of range"""
    sx, sy, ss = sensor(cfg, pose, sensor_xyz)
    if ss is None:
        return 0, [], None
    cls, cx, cy, s = er.point_classes(cfg, points, pose, sensor_xyz)
    with np.errstate(all="ignore"):
        eligible = (cls != er.SKIPPED) & (s >= S_MIN) & (s <= S_MAX)
    if not eligible.any():
        return 0, [], ss
    dx, dy, es = cx[eligible] - sx, cy[eligible] - sy, s[eligible]
    return int(eligible.sum()), sorted({(int(a), int(b), int(c)) for a, b, c in zip(dx, dy, es)}), ss


def ray_slab(ss, es, m, j):
    """u(j), in Python integers"""
    d = es - ss
    return ss + (1 if d > 0 else -1 if d < 0 else 0) * ((j * abs(d) + m) // (2 * m))


def step_mask(ss, es, m, k, W):
    """the mask of step k of the ray, a Python integer"""
    a, b = ray_slab(ss, es, m, max(2 * k - 1, 0)), ray_slab(ss, es, m, 2 * k + 1)
    lo, hi = min(a, b) - W, max(a, b) + W
    return sum(1 << bit for bit in range(max(lo, 0), min(hi, 63) + 1))  # empty when hi < 0 or lo > 63


def steps(cfg, points, pose, sensor_xyz, G, W, spans=False):
    """every step of every ray of the frame -> (carve_points, gx[t], gy[t], mask[t] uint64): grid cells (int64, inside the grid or not)
    and masks; spans: (lo[t], hi[t]) instead, before they are cut to the column"""
    n, tri, ss = triples(cfg, points, pose, sensor_xyz)
    empty = np.zeros(0, dtype=np.int64)
    if spans and (not tri or all(max(abs(a), abs(b)) <= int(G) for a, b, _ in tri)):
        return empty, empty
    if not tri:
        return n, empty, empty, np.zeros(0, dtype=U64)
    sx, sy, _ = sensor(cfg, pose, sensor_xyz)
    t = np.array(tri, dtype=np.int64)
    dx, dy, es = t[:, 0], t[:, 1], t[:, 2]
    m = np.maximum(np.abs(dx), np.abs(dy))
    count = np.maximum(m - int(G), 0)  # steps k = 0 .. m - 1 - G
    ray = np.repeat(np.arange(len(t)), count)
    if len(ray) == 0:
        return n, empty, empty, np.zeros(0, dtype=U64)
    k = np.arange(len(ray)) - np.repeat(np.cumsum(count) - count, count)
    dx, dy, es, m = dx[ray], dy[ray], es[ray], m[ray]
    gx = int(sx) + np.sign(dx) * ((2 * k * np.abs(dx) + m) // (2 * m))
    gy = int(sy) + np.sign(dy) * ((2 * k * np.abs(dy) + m) // (2 * m))
    d = es - ss

    def u(j):
        return ss + np.sign(d) * ((j * np.abs(d) + m) // (2 * m))

    a, b = u(np.maximum(2 * k - 1, 0)), u(2 * k + 1)
    lo, hi = np.minimum(a, b) - int(W), np.maximum(a, b) + int(W)
    if spans:
        return lo, hi
    first, last = np.clip(lo, 0, 63).astype(U64), np.clip(hi, 0, 63).astype(U64)
    mask = (U64(FULL) << first) & (U64(FULL) >> (U64(63) - last))
    mask[(hi < 0) | (lo > 63)] = U64(0)
    return n, gx, gy, mask


def carve(cfg, columns, points, pose, sensor_xyz, G, W, keep_ground):
    """the carve of one frame in `columns` (uint64 [height, width], changed in place) -> (carve_points, bits_cleared, cells_emptied)"""
    n, gx, gy, mask = steps(cfg, points, pose, sensor_xyz, G, W)
    inside = (gx >= 0) & (gx < cfg["width"]) & (gy >= 0) & (gy < cfg["height"])
    M = np.zeros(cfg["height"] * cfg["width"], dtype=U64)  # the OR of the masks of all steps that visit a cell
    np.bitwise_or.at(M, gy[inside] * cfg["width"] + gx[inside], mask[inside])
    bits_cleared = cells_emptied = 0
    flat = columns.reshape(-1)
    for i in np.flatnonzero(M):
        c, clear = int(flat[i]), int(M[i])
        keep = (c & -c) if keep_ground else 0
        after = c & ~(clear & ~keep) & FULL
        bits_cleared += bin(c & ~after).count("1")
        cells_emptied += c != 0 and after == 0
        flat[i] = U64(after)
    return n, bits_cleared, cells_emptied


def update(cfg, columns, points, pose, sensor_xyz, G, W, keep_ground):
    """an UPDATE: the carve, then the mark -> the nine words"""
    carved = carve(cfg, columns, points, pose, sensor_xyz, G, W, keep_ground)
    return er.integrate(cfg, columns, points, pose, sensor_xyz) + carved
