"""numpy restatement of the depth view's semantics (include/kicp.h, kicp_view_*, kicp_map_remove_seen_through): the image of a frame,
the verdict for world points and the sweep of a map.  Everything is exact: the tests compare with np.array_equal.

The transform is kicp_se3.hpp's quat_rotate restated operation by operation in IEEE doubles (numpy fuses nothing); the image is a
minimum over a set (np.minimum.at), so it cannot depend on the order of the points."""
import numpy as np

SEEN_THROUGH, IN_RANGE = 1, 2


def make_config(res, window, min_rays, max_ray, margin, margin_per_metre):
    return dict(res=int(res), window=int(window), min_rays=int(min_rays), max_ray=float(max_ray), margin=float(margin),
                margin_per_metre=float(margin_per_metre))


def transform(pose, points):
    """pose * p: p + w (2 v x p) + v x (2 v x p), then + t - the map update's own transform"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    qx, qy, qz, qw, tx, ty, tz = (np.float64(v) for v in pose)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        ux, uy, uz = qy * z - qz * y, qz * x - qx * z, qx * y - qy * x
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        ox = x + qw * ux + (qy * uz - qz * uy)
        oy = y + qw * uy + (qz * ux - qx * uz)
        oz = z + qw * uz + (qx * uy - qy * ux)
        return np.stack([ox + tx, oy + ty, oz + tz], axis=1)


def sensor_world(pose, sensor_xyz):
    """c = pose * sensor_xyz; NaN when the pose or the sensor is not finite"""
    pose, s = np.asarray(pose, dtype=np.float64).reshape(7), np.asarray(sensor_xyz, dtype=np.float64).reshape(3)
    if not (np.all(np.isfinite(pose)) and np.all(np.isfinite(s))):
        return np.full(3, np.nan)
    return transform(pose, s)[0]


def project(cfg, v):
    """offsets from the sensor [n, 3] -> (ok[n], m[n], face[n], u[n], w[n]); the last three are only meaningful where ok"""
    res = cfg["res"]
    with np.errstate(all="ignore"):
        a3 = np.abs(v)
        ax, ay, az = a3[:, 0], a3[:, 1], a3[:, 2]
        m = np.maximum(np.maximum(ax, ay), az)
        ok = np.isfinite(ax) & np.isfinite(ay) & np.isfinite(az) & (0.0 < m) & (m <= cfg["max_ray"])
        on_x, on_y = ax == m, ay == m
        axis = np.where(on_x, 0, np.where(on_y, 1, 2))
        comp = v[np.arange(len(v)), axis]
        face = 2 * axis + (comp < 0.0)
        a = np.where(on_x, v[:, 1], v[:, 0])
        b = np.where(on_x | on_y, v[:, 2], v[:, 1])
        half = res / 2.0
        fu, fw = np.floor((a / m + 1.0) * half), np.floor((b / m + 1.0) * half)
    u = np.minimum(res - 1, np.where(ok, fu, 0).astype(np.int64))
    w = np.minimum(res - 1, np.where(ok, fw, 0).astype(np.int64))
    return ok, m, face.astype(np.int64), u, w


def render(cfg, points, pose, sensor_xyz):
    """one frame -> (depth float32 [6, res, res], (used, skipped), c)"""
    res = cfg["res"]
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    c = sensor_world(pose, sensor_xyz)
    depth = np.full((6, res, res), np.inf, dtype=np.float32)
    if not np.all(np.isfinite(c)):
        return depth, (0, len(p)), c
    w = transform(pose, p)
    with np.errstate(all="ignore"):
        ok, m, face, u, w_ = project(cfg, w - c)
    ok &= np.all(np.isfinite(p), axis=1) & np.all(np.isfinite(w), axis=1)
    with np.errstate(over="ignore"):
        np.minimum.at(depth.reshape(-1), ((face * res + w_) * res + u)[ok], m[ok].astype(np.float32))
    used = int(ok.sum())
    return depth, (used, len(p) - used), c


def verdict(cfg, depth, c, points):
    """world points -> uint8 per point: bit 0 seen through, bit 1 in range"""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    res, win = cfg["res"], cfg["window"]
    with np.errstate(all="ignore"):
        ok, m, face, u, w_ = project(cfg, q - np.asarray(c, dtype=np.float64))
    count = np.zeros(len(q), dtype=np.int64)
    nearest = np.full(len(q), np.inf, dtype=np.float32)
    for dw in range(-win, win + 1):
        for du in range(-win, win + 1):
            iu, iw = u + du, w_ + dw
            inside = (iu >= 0) & (iu < res) & (iw >= 0) & (iw < res)  # the same face only
            d = np.where(inside, depth[face, np.clip(iw, 0, res - 1), np.clip(iu, 0, res - 1)], np.float32(np.inf))
            count += d != np.inf
            nearest = np.minimum(nearest, d)
    with np.errstate(all="ignore"):
        through = ok & (count >= cfg["min_rays"]) & (m + (cfg["margin"] + cfg["margin_per_metre"] * m) < nearest.astype(np.float64))
    return (ok * IN_RANGE + through * SEEN_THROUGH).astype(np.uint8)


def sweep(cfg, depth, c, cloud, vs):
    """the map whose points are `cloud` (any order that keeps each bucket's order, e.g. mapdev_ref.bucket_sorted) swept
    -> (keep mask [n], (points in range, points removed, voxels that lost at least one point, voxels erased))"""
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    v = verdict(cfg, depth, c, cloud)
    gone = (v & SEEN_THROUGH) != 0
    key = np.floor(cloud / vs)
    voxels, inverse = np.unique(key, axis=0, return_inverse=True) if len(cloud) else (np.zeros((0, 3)), np.zeros(0, dtype=np.int64))
    inverse = np.asarray(inverse).reshape(-1)
    lost = np.bincount(inverse[gone], minlength=len(voxels))
    held = np.bincount(inverse, minlength=len(voxels))
    return ~gone, (int(((v & IN_RANGE) != 0).sum()), int(gone.sum()), int((lost > 0).sum()), int(((lost > 0) & (lost == held)).sum()))
