"""A numpy restatement of the whole-map relocalisation's integer parts (include/kicp.h: kicp_occ_build, kicp_occ_score_nodes,
kicp_search_poses): the occupancy pyramid as bool arrays [z, y, x] and as the packed words kicp_occ_level downloads, the cells of a
frame per yaw, node scores, and the exhaustive top-M with the (hits descending, index ascending) rule.  Everything is fp64 in the
header's operation order (numpy does not contract) and integer from the floor on, so the GPU must agree exactly.  The rotation
table is an INPUT: feed it K.search_yaws(window), the very doubles the device uses."""
import numpy as np


def geometry(points, cell, dilate):
    """-> (min[3], dims[3]); an empty map: zeros and ones"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(points) == 0:
        return np.zeros(3), np.ones(3, dtype=np.int64)
    mn = (np.floor(points.min(axis=0) / cell) - float(dilate + 1)) * cell
    dims = np.floor((points.max(axis=0) - mn) / cell) + float(dilate + 2)
    return mn, dims.astype(np.int64)


def cells_of(values, mn, cell):
    return np.floor((values - mn) / cell).astype(np.int64)


def pyramid(points, cell, dilate, levels):
    """-> (min, dims, [level 0 .. levels] bool arrays shaped [z, y, x])"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    mn, dims = geometry(points, cell, dilate)
    occ = np.zeros((dims[2], dims[1], dims[0]), dtype=bool)
    if len(points):
        c = cells_of(points, mn, cell)
        for dz in range(-dilate, dilate + 1):
            for dy in range(-dilate, dilate + 1):
                for dx in range(-dilate, dilate + 1):
                    x, y, z = c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz
                    ok = (x >= 0) & (x < dims[0]) & (y >= 0) & (y < dims[1]) & (z >= 0) & (z < dims[2])
                    occ[z[ok], y[ok], x[ok]] = True
    out = [occ]
    for h in range(1, levels + 1):
        s, prev = 1 << (h - 1), out[-1]
        nxt = prev.copy()
        if s < dims[0]:
            nxt[:, :, :-s] |= prev[:, :, s:]
        if s < dims[1]:
            nxt[:, :-s, :] |= prev[:, s:, :]
        if s < dims[0] and s < dims[1]:
            nxt[:, :-s, :-s] |= prev[:, s:, s:]
        out.append(nxt)
    return mn, dims, out


def pack(level):
    """a level as kicp_occ_level's words, shaped [z, y, words per row]: cell x is bit x & 31 of word x >> 5"""
    dz, dy, dx = level.shape
    wx = (dx + 31) // 32
    padded = np.zeros((dz, dy, wx * 32), dtype=np.uint8)
    padded[:, :, :dx] = level
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<u4").reshape(dz, dy, wx)


def frame_cells(frame, cs, window, mn, cell):
    """the cell of every frame point at every yaw -> int64 [nyaw, n, 3]; window: an object with x0, y0, z"""
    p = np.asarray(frame, dtype=np.float64).reshape(-1, 3)
    c, s = cs[:, 0][:, None], cs[:, 1][:, None]
    px, py, pz = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    with np.errstate(invalid="ignore"):
        x = np.floor((((c * px - s * py) + window.x0) - mn[0]) / cell)
        y = np.floor((((s * px + c * py) + window.y0) - mn[1]) / cell)
        z = np.floor(((pz + window.z) - mn[2]) / cell) + np.zeros_like(x)
    out = np.stack([x, y, z], axis=-1)
    return np.where(np.isfinite(out) & (np.abs(out) < 2.0 ** 40), out, -2.0 ** 40).astype(np.int64)


def score_nodes(level, cells, window, nodes, h=0):
    """scores of node indices against one bool level (level h of the pyramid): points whose shifted cell is set; cells outside the grid
    are empty, except that at level h an x or y in -2^h < x < 0 reads column / row 0 (include/kicp.h)"""
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    nx, ny = int(window.nx), int(window.ny)
    ix, row = nodes % nx, nodes // nx
    iy, j = row % ny, row // ny
    dz, dy, dx = level.shape
    out = np.zeros(len(nodes), dtype=np.uint32)
    for k in range(len(nodes)):
        c = cells[j[k]]
        x, y, z = c[:, 0] + ix[k], c[:, 1] + iy[k], c[:, 2]
        x, y = np.where((x < 0) & (x > -(1 << h)), 0, x), np.where((y < 0) & (y > -(1 << h)), 0, y)
        ok = (x >= 0) & (x < dx) & (y >= 0) & (y < dy) & (z >= 0) & (z < dz)
        out[k] = int(level[z[ok], y[ok], x[ok]].sum())
    return out


def score_window(level, cells, window):
    """the scores of ALL nodes of the window -> uint32 [nyaw, ny, nx] (node index = its flat index): per point, the slab of the level
    its cell sweeps while (ix, iy) runs over the window is added to the yaw's plane"""
    nx, ny, nyaw = int(window.nx), int(window.ny), int(window.nyaw)
    dz, dy, dx = level.shape
    lvl = level.astype(np.uint16)
    out = np.zeros((nyaw, ny, nx), dtype=np.uint32)
    for j in range(nyaw):
        plane = np.zeros((ny, nx), dtype=np.uint16)
        for cx, cy, cz in cells[j]:
            if not 0 <= cz < dz:
                continue
            x0, x1, y0, y1 = max(cx, 0), min(cx + nx, dx), max(cy, 0), min(cy + ny, dy)
            if x0 < x1 and y0 < y1:
                plane[y0 - cy:y1 - cy, x0 - cx:x1 - cx] += lvl[cz, y0:y1, x0:x1]
        out[j] = plane
    return out


def top_m(scores, m):
    """the first min(m, all) nodes by (score descending, node index ascending) -> (nodes int64, hits uint32)"""
    flat = np.asarray(scores).reshape(-1)
    order = np.argsort(-flat.astype(np.int64), kind="stable")[:min(int(m), flat.size)]
    return order.astype(np.int64), flat[order].astype(np.uint32)


def node_pose(window, cell, node):
    """the pose [qx, qy, qz, qw, tx, ty, tz] of a node index"""
    nx, ny = int(window.nx), int(window.ny)
    ix, row = int(node) % nx, int(node) // nx
    iy, j = row % ny, row // ny
    yaw = window.yaw0 + float(j) * window.yaw_step
    return np.array([0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw), window.x0 + float(ix) * cell, window.y0 + float(iy) * cell, window.z])
