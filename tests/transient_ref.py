"""The transient obstacles of include/kicp.h ("what stands in known free space right now") restated in numpy and Python integers: the
used points' endpoint cells from tests/grid_ref.py, n(c) by a histogram, the transient-cell test on the readout of tests/grid_ref.py, the
components two ways as tests/frontier_ref.py finds them - a breadth-first flood fill and min-label sweeps, which must agree - and the
ten words per transient from the labelled cells."""
import numpy as np

import frontier_ref as fr
import grid_ref

NONE = fr.NONE
WORDS = 10


def returns(cfg, points, pose, sensor_xyz):
    """-> (n(c) as int64 (H, W), (points used, used points whose endpoint cell lies inside the grid, cells with n(c) > 0), the sensor's
    cell (sx, sy) as Python ints, or None when it is not finite - then no point is used)"""
    used, offs, (sx, sy) = grid_ref.endpoints(cfg, points, pose, sensor_xyz)
    W, H = cfg["width"], cfg["height"]
    n = np.zeros((H, W), dtype=np.int64)
    if not len(offs):
        return n, (0, 0, 0), ((int(sx), int(sy)) if np.isfinite(sx) and np.isfinite(sy) else None)
    sxi, syi = int(sx), int(sy)
    gx, gy = sxi + offs[:, 0], syi + offs[:, 1]
    ok = (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)
    np.add.at(n, (gy[ok], gx[ok]), 1)
    return n, (int(used.sum()), int(ok.sum()), int((n > 0).sum())), (sxi, syi)


def transient_cells(counts, n, min_observations=1, free_max=65, min_points=1):
    v = grid_ref.occupancy(counts, min_observations).astype(np.int64)
    return (n >= min_points) & (v >= 0) & (v <= free_max)


def rows_of(labels, n, sensor, min_size=1):
    """uint64 (T, 10) from a label plane: label, size, returns, sum n x, sum n y, min x, max x, min y, max y, and the least key
    d2 * 2^32 + index; transients below min_size dropped, ascending labels"""
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
        sx, sy = sensor
        key = min((((x - sx) ** 2 + (y - sy) ** 2) << 32) + y * W + x for x, y in cells)
        cn = [int(n[y, x]) for x, y in cells]
        cx, cy = [c[0] for c in cells], [c[1] for c in cells]
        out.append([label, len(cells), sum(cn), sum(k * x for k, x in zip(cn, cx)), sum(k * y for k, y in zip(cn, cy)), min(cx), max(cx), min(cy), max(cy), key])
    return np.array(out, dtype=np.uint64).reshape(-1, WORDS)


def plane_of(labels, min_size=1):
    """uint8 (H, W): 1 on the cells of the transients of at least min_size cells"""
    flat = labels.ravel()
    sizes = np.bincount(flat[flat != NONE].astype(np.int64), minlength=flat.size)
    plane = np.zeros(flat.size, dtype=np.uint8)
    on = flat != NONE
    plane[on] = sizes[flat[on].astype(np.int64)] >= min_size
    return plane.reshape(labels.shape)


def transients(cfg, counts, points, pose, sensor_xyz, min_observations=1, free_max=65, min_points=1, min_size=1, sweeps=False):
    """-> (rows uint64 (T, 10), labels uint32 (H, W), plane uint8 (H, W), the four statistics); sweeps: the components by the min-label
    sweeps instead of the flood fill"""
    n, stats, sensor = returns(cfg, points, pose, sensor_xyz)
    flags = transient_cells(counts, n, min_observations, free_max, min_points)
    labels = fr.labels_sweeps(flags) if sweeps else fr.labels_flood(flags)
    return rows_of(labels, n, sensor, min_size), labels, plane_of(labels, min_size), stats + (int(flags.sum()),)


def patched_readout(counts, plane, min_observations=1):
    """the readout with the plane's cells set to 100: what the switch makes of a grid for occupied_thresh < 1"""
    occ = grid_ref.occupancy(counts, min_observations)
    occ[np.asarray(plane, dtype=bool)] = 100
    return occ
