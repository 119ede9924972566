"""numpy restatement of the height columns' semantics (include/kicp.h, kicp_elev_*), written from the header's text: the classes of a
frame's points, the columns and the six statistics of a frame, and the traversability of a layer.  Everything is exact: the tests
compare with np.array_equal.

The transform is pose_to_rt of kicp_se3.hpp restated operation by operation in Python floats (rows 0 and 1: grid_ref.pose_to_rt; row
2 here).  Columns are Python integers inside integrate() and classify() - no shift of a fixed-width word can go wrong there - and
uint64 arrays outside."""
import math

import numpy as np

import clearance_ref as cr
import grid_ref as gr

SKIPPED, OUTSIDE_GRID, OUTSIDE_COLUMN, USED = 0, 1, 2, 3


def make_config(cell, origin_x, origin_y, width, height, z_origin, slab, max_ray):
    return dict(cell=float(cell), origin_x=float(origin_x), origin_y=float(origin_y), width=int(width), height=int(height), z_origin=float(z_origin),
                slab=float(slab), max_ray=float(max_ray), reach=int(math.ceil(float(max_ray) / float(cell))))


def row2(pose):
    """row 2 of R and of t, as kicp_se3.hpp's pose_to_rt forms them"""
    qx, qy, qz, qw = (float(v) for v in pose[:4])
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy = tx * qw, ty * qw
    txx, txz = tx * qx, tz * qx
    tyy, tyz = ty * qy, tz * qy
    return (txz - twy, tyz + twx, 1 - (txx + tyy)), float(pose[6])


def point_classes(cfg, points, pose, sensor_xyz):
    """-> (class[n], cx[n], cy[n], s[n]): cx, cy, s are meaningful (and integer valued) where the class is USED"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    r0, r1, t0, t1 = gr.pose_to_rt(pose)
    r2, t2 = row2(pose)
    with np.errstate(all="ignore"):
        sen = np.asarray(sensor_xyz, dtype=np.float64).reshape(3)
        sx = gr._cell(np.float64(gr._world(r0, t0, sen[0], sen[1], sen[2])), cfg["origin_x"], cfg["cell"])
        sy = gr._cell(np.float64(gr._world(r1, t1, sen[0], sen[1], sen[2])), cfg["origin_y"], cfg["cell"])
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        wx, wy, wz = gr._world(r0, t0, x, y, z), gr._world(r1, t1, x, y, z), gr._world(r2, t2, x, y, z)
        cx, cy = gr._cell(wx, cfg["origin_x"], cfg["cell"]), gr._cell(wy, cfg["origin_y"], cfg["cell"])
        s = np.floor((wz - cfg["z_origin"]) / cfg["slab"])
        kept = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(wx) & np.isfinite(wy) & np.isfinite(wz)
        kept &= (np.abs(cx - sx) <= cfg["reach"]) & (np.abs(cy - sy) <= cfg["reach"])  # (a NaN compares false)
        in_grid = (cx >= 0) & (cx < cfg["width"]) & (cy >= 0) & (cy < cfg["height"])
        in_column = (s >= 0) & (s <= 63)
    cls = np.full(len(p), SKIPPED)
    cls[kept & ~in_grid] = OUTSIDE_GRID
    cls[kept & in_grid & ~in_column] = OUTSIDE_COLUMN
    cls[kept & in_grid & in_column] = USED
    return cls, cx, cy, s


def integrate(cfg, columns, points, pose, sensor_xyz):
    """one frame into `columns` (uint64 [height, width], changed in place) -> (used, skipped, outside_grid, outside_column, new_bits,
    new_cells)"""
    cls, cx, cy, s = point_classes(cfg, points, pose, sensor_xyz)
    used = cls == USED
    pairs = {(int(b), int(a), int(c)) for a, b, c in zip(cx[used], cy[used], s[used])}  # the SET of (iy, ix, slab)
    new_bits = sum(1 for iy, ix, b in pairs if not (int(columns[iy, ix]) >> b) & 1)
    new_cells = len({(iy, ix) for iy, ix, _ in pairs if int(columns[iy, ix]) == 0})
    for iy, ix, b in pairs:
        columns[iy, ix] = np.uint64(int(columns[iy, ix]) | (1 << b))
    return tuple(int((cls == k).sum()) for k in (USED, SKIPPED, OUTSIDE_GRID, OUTSIDE_COLUMN)) + (new_bits, new_cells)


def window(cfg, pose, sensor_xyz):
    """kicp_elev_last_window after this frame: the grid's rule (clearance_ref.window) on the layer's plane"""
    return cr.window(dict(cfg, z_min=-np.inf, z_max=np.inf), pose, sensor_xyz)


def classify(columns, step_slabs, robot_slabs):
    """-> (classes int8 [H, W]: -1 unknown, 0 traversable, 100 obstacle; ground uint8 [H, W], 255 unknown; body bool; step bool)"""
    cols = np.asarray(columns, dtype=np.uint64)
    H, W = cols.shape
    S, R = int(step_slabs), int(robot_slabs)
    assert 0 <= S <= 62 and S < R <= 64
    ground = np.full((H, W), 255, dtype=np.uint8)
    body, step = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            c = int(cols[y, x])
            if c:
                g = (c & -c).bit_length() - 1
                ground[y, x] = g
                body[y, x] = any((c >> b) & 1 for b in range(g + S + 1, min(g + R, 63) + 1))
    g16 = ground.astype(np.int64)
    padded = np.full((H + 2, W + 2), 255, dtype=np.int64)
    padded[1:-1, 1:-1] = g16
    known = g16 != 255
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dx, dy) != (1, 1):
                n = padded[dy:dy + H, dx:dx + W]
                step |= known & (n != 255) & (g16 - n > S)
    classes = np.where(~known, -1, np.where(body | step, 100, 0)).astype(np.int8)
    return classes, ground, body, step


def counts(classes, body):
    """(unknown, traversable, BODY, STEP only)"""
    return (int((classes == -1).sum()), int((classes == 0).sum()), int(body.sum()), int(((classes == 100) & ~body).sum()))


def restrict(a, rect):
    x0, y0, w, h = rect
    return a[y0:y0 + h, x0:x0 + w]
