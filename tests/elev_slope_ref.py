"""numpy restatement of the height columns' slope limit (include/kicp.h, THE SLOPE LIMIT), written from the header's text: the nine
sums over every cell's fit set, the determinants D, Da, Db, the predicate, the classes and the five counts.  BODY and STEP are
elev_ref.classify's.  The sums are int64 arrays (they stay below 2^17); from the determinants on everything is Python integers in
object arrays, so no width can go wrong here.  Everything is exact: the tests compare with np.array_equal."""
from types import SimpleNamespace

import numpy as np

import elev_ref as er

NAMES = ("n", "sx", "sy", "sxx", "sxy", "syy", "sz", "sxz", "syz")


def check_config(slope):
    L, K, min_cells, rise, run = (int(v) for v in slope)
    assert 1 <= L <= 8 and 0 <= K <= 63 and 3 <= min_cells <= 289 and 0 <= rise <= 65535 and 1 <= run <= 65535
    return L, K, min_cells, rise, run


def sums(ground, L, K):
    """-> dict of int64 [H, W]: the nine sums over the fit set of every known cell (zeros for an unknown one)"""
    H, W = ground.shape
    g = ground.astype(np.int64)
    known = ground != 255
    padded = np.full((H + 2 * L, W + 2 * L), 255, dtype=np.int64)  # cells outside the grid: like unknown ones
    padded[L:L + H, L:L + W] = g
    s = {name: np.zeros((H, W), dtype=np.int64) for name in NAMES}
    for dy in range(-L, L + 1):
        for dx in range(-L, L + 1):
            n = padded[L + dy:L + dy + H, L + dx:L + dx + W]
            m = known & (n != 255) & (np.abs(n - g) <= K)
            z = np.where(m, n - g, 0)
            mi = m.astype(np.int64)
            for name, v in (("n", mi), ("sx", mi * dx), ("sy", mi * dy), ("sxx", mi * dx * dx), ("sxy", mi * dx * dy), ("syy", mi * dy * dy), ("sz", z),
                            ("sxz", z * dx), ("syz", z * dy)):
                s[name] += v
    return s


def determinants(s):
    """-> (D, Da, Db), object arrays of Python integers"""
    n, Sx, Sy, Sxx, Sxy, Syy, Sz, Sxz, Syz = (s[name].astype(object) for name in NAMES)
    D = Sxx * (Syy * n - Sy * Sy) - Sxy * (Sxy * n - Sy * Sx) + Sx * (Sxy * Sy - Syy * Sx)
    Da = Sxz * (Syy * n - Sy * Sy) - Sxy * (Syz * n - Sy * Sz) + Sx * (Syz * Sy - Syy * Sz)
    Db = Sxx * (Syz * n - Sz * Sy) - Sxz * (Sxy * n - Sy * Sx) + Sx * (Sxy * Sz - Syz * Sx)
    return D, Da, Db


def sides(D, Da, Db, rise, run):
    """the two sides of the comparison, Python integers: SLOPE is left > right"""
    return (Da * Da + Db * Db) * (int(run) * int(run)), D * D * (int(rise) * int(rise))


def classify(columns, step_slabs, robot_slabs, slope):
    """-> namespace: classes int8 [H, W] (-1 unknown, 0 traversable, 100 BODY, STEP or SLOPE), ground uint8, fit int64 [H, W, 3] (D, Da,
    Db; zeros without a fit), body, step, has_fit, slope (bool), sums (dict), D, Da, Db (object arrays, of every cell)"""
    L, K, min_cells, rise, run = check_config(slope)
    _, ground, body, step = er.classify(columns, step_slabs, robot_slabs)
    known = ground != 255
    s = sums(ground, L, K)
    D, Da, Db = determinants(s)
    has_fit = known & (s["n"] >= min_cells) & (D > 0).astype(bool)
    left, right = sides(D, Da, Db, rise, run)
    steep = has_fit & (left > right).astype(bool)
    fit = np.stack([np.where(has_fit, v, 0).astype(np.int64) for v in (D, Da, Db)], axis=-1)
    classes = np.where(~known, -1, np.where(body | step | steep, 100, 0)).astype(np.int8)
    return SimpleNamespace(classes=classes, ground=ground, fit=fit, body=body, step=step, has_fit=has_fit, slope=steep, sums=s, D=D, Da=Da, Db=Db, left=left, right=right)


def counts(c, rect=None):
    """(unknown, traversable, BODY, STEP only, SLOPE only) of a classify() result, of `rect` = (x0, y0, w, h) or of the full layer"""
    r = (lambda a: er.restrict(a, rect)) if rect is not None else (lambda a: a)
    classes, body, step, steep = r(c.classes), r(c.body), r(c.step), r(c.slope)
    return (int((classes == -1).sum()), int((classes == 0).sum()), int(body.sum()), int((step & ~body).sum()), int((steep & ~body & ~step).sum()))


def slope_limit(cell, slab, max_tangent):
    """kicp_elev_slope_limit: (rise_slabs, run_cells), each operation rounded on its own; None where the entry refuses"""
    with np.errstate(all="ignore"):
        rise = np.floor(((np.float64(max_tangent) * np.float64(cell)) / np.float64(slab)) * np.float64(1024.0))
    return (int(rise), 1024) if np.isfinite(rise) and 0 <= rise <= 65535 else None
