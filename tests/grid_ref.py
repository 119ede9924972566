"""numpy restatement of the 2-D occupancy grid's semantics (include/kicp.h, kicp_grid_*): the per-frame update, the readout and the
bytes of the map files.  Everything is exact: the tests compare with np.array_equal.

The transform is pose_to_rt of kicp_se3.hpp restated operation by operation in Python floats (IEEE doubles, no fused operations);
the ray walk is in closed form, so one ray is a pair of arrays over k."""
import math
import os

import numpy as np


def make_config(cell, origin_x, origin_y, width, height, z_min, z_max, max_ray):
    return dict(cell=float(cell), origin_x=float(origin_x), origin_y=float(origin_y), width=int(width), height=int(height), z_min=float(z_min),
                z_max=float(z_max), max_ray=float(max_ray), reach=int(math.ceil(float(max_ray) / float(cell))))


def pose_to_rt(pose):
    """rows 0 and 1 of R and of t, as kicp_se3.hpp's pose_to_rt forms them"""
    qx, qy, qz, qw, t0, t1 = (float(v) for v in pose[:6])
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    row0 = (1 - (tyy + tzz), txy - twz, txz + twy)
    row1 = (txy + twz, 1 - (txx + tzz), tyz - twx)
    return row0, row1, t0, t1


def _world(row, t, x, y, z):
    return ((row[0] * x + row[1] * y) + row[2] * z) + t


def _cell(w, origin, cell):
    return np.floor((w - origin) / cell)


def walk(dx, dy):
    """offsets from the sensor's cell of the m = max(|dx|, |dy|) cells the ray to the endpoint offset (dx, dy) visits -> (ox[m], oy[m])"""
    a, b = abs(int(dx)), abs(int(dy))
    m = max(a, b)
    k = np.arange(m, dtype=np.int64)
    if m == 0:
        return k, k
    return int(np.sign(dx)) * ((2 * k * a + m) // (2 * m)), int(np.sign(dy)) * ((2 * k * b + m) // (2 * m))


def endpoints(cfg, points, pose, sensor_xyz):
    """-> (used mask[n], offsets (dx, dy) of the used points' endpoint cells from the sensor's cell as int64 [n_used, 2], sensor cell
    (sx, sy) as floats - integer valued, or not finite)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    row0, row1, t0, t1 = pose_to_rt(pose)
    with np.errstate(all="ignore"):
        s = np.asarray(sensor_xyz, dtype=np.float64).reshape(3)
        sx = _cell(np.float64(_world(row0, t0, s[0], s[1], s[2])), cfg["origin_x"], cfg["cell"])
        sy = _cell(np.float64(_world(row1, t1, s[0], s[1], s[2])), cfg["origin_y"], cfg["cell"])
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        used = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (cfg["z_min"] <= z) & (z < cfg["z_max"])
        wx, wy = _world(row0, t0, x, y, z), _world(row1, t1, x, y, z)
        used &= np.isfinite(wx) & np.isfinite(wy)
        ox, oy = _cell(wx, cfg["origin_x"], cfg["cell"]) - sx, _cell(wy, cfg["origin_y"], cfg["cell"]) - sy
        used &= (np.abs(ox) <= cfg["reach"]) & (np.abs(oy) <= cfg["reach"])  # (a NaN compares false)
    return used, np.stack([ox[used], oy[used]], axis=1).astype(np.int64), (float(sx), float(sy))


def integrate(cfg, counts, points, pose, sensor_xyz):
    """one frame into `counts` (uint16 [height, width, 2], changed in place) -> (used, skipped, cells HIT, cells MISS)"""
    used, offs, (sx, sy) = endpoints(cfg, points, pose, sensor_xyz)
    n_used = int(used.sum())
    stats = [n_used, int(len(used)) - n_used, 0, 0]
    if n_used == 0:
        return tuple(stats)
    W, H = cfg["width"], cfg["height"]
    sxi, syi = int(sx), int(sy)  # finite: a point was used
    hit, miss = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)

    def mark(plane, gx, gy):
        ok = (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)
        plane[gy[ok], gx[ok]] = True

    unique = np.unique(offs, axis=0)
    mark(hit, sxi + unique[:, 0], syi + unique[:, 1])
    for dx, dy in unique:
        ox, oy = walk(dx, dy)
        mark(miss, sxi + ox, syi + oy)
    miss &= ~hit
    for plane, which in ((hit, 0), (miss, 1)):
        c = counts[:, :, which]
        c[plane] = np.minimum(c[plane].astype(np.int64) + 1, 65535).astype(np.uint16)
    stats[2], stats[3] = int(hit.sum()), int(miss.sum())
    return tuple(stats)


def occupancy(counts, min_observations=1):
    c = np.asarray(counts, dtype=np.int64)
    hits, seen = c[..., 0], c[..., 0] + c[..., 1]
    out = np.full(seen.shape, -1, dtype=np.int8)
    known = (seen >= min_observations) & (seen > 0)
    out[known] = ((100 * hits[known] + seen[known] // 2) // seen[known]).astype(np.int8)
    return out


def map_files(prefix, occ, cell, origin_x, origin_y, occupied_thresh=0.65, free_thresh=0.25):
    """-> (the bytes of <prefix>.pgm, the text of <prefix>.yaml) for occ = int8 [height, width]"""
    occ = np.asarray(occ, dtype=np.int8)
    h, w = occ.shape
    v = occ.astype(np.float64)
    pix = np.full(occ.shape, 205, dtype=np.uint8)
    pix[(occ >= 0) & (v < free_thresh * 100.0)] = 254
    pix[v > occupied_thresh * 100.0] = 0
    pgm = b"P5\n%d %d\n255\n" % (w, h) + pix[::-1].tobytes()
    yaml = ("image: %s\nmode: trinary\nresolution: %.17g\norigin: [%.17g, %.17g, 0]\nnegate: 0\noccupied_thresh: %.17g\nfree_thresh: %.17g\n"
            % (os.path.basename(prefix) + ".pgm", cell, origin_x, origin_y, occupied_thresh, free_thresh))
    return pgm, yaml
