"""numpy restatement of the height columns' class ROUGH (include/kicp.h, ROUGH) and of the fill of a grid's unknown cells from another
grid (include/kicp.h, THE FILL), written from the header's text.  ROUGH: the slope limit's fit (tests/elev_slope_ref.py: the nine sums,
D, Da, Db, "has a fit", SLOPE), a tenth sum Szz, the intercept's determinant Dc, the residual Q and the predicate Q den > num n D, in
Python integers from the determinants on, so no width can go wrong here.  Everything is exact: the tests compare with np.array_equal."""
from types import SimpleNamespace

import numpy as np

import elev_ref as er
import elev_slope_ref as sr


def check_rough(rough):
    num, den = (int(v) for v in rough)
    assert 0 <= num <= 65535 and 1 <= den <= 65535
    return num, den


def szz(ground, L, K, admit_beyond_gate=False):
    """-> int64 [H, W]: the sum of z^2 over the fit set of every known cell.  admit_beyond_gate: what a gate that Szz forgot would sum -
    every known window cell - for the cases test."""
    H, W = ground.shape
    g = ground.astype(np.int64)
    known = ground != 255
    padded = np.full((H + 2 * L, W + 2 * L), 255, dtype=np.int64)
    padded[L:L + H, L:L + W] = g
    out = np.zeros((H, W), dtype=np.int64)
    for dy in range(-L, L + 1):
        for dx in range(-L, L + 1):
            n = padded[L + dy:L + dy + H, L + dx:L + dx + W]
            m = known & (n != 255) & ((np.abs(n - g) <= K) | admit_beyond_gate)
            z = np.where(m, n - g, 0)
            out += z * z
    return out


def residual(s, Szz, D, Da, Db):
    """-> (Q, Dc), object arrays of Python integers"""
    n, Sx, Sy, Sxx, Sxy, Syy, Sz, Sxz, Syz = (s[name].astype(object) for name in sr.NAMES)
    Dc = Sxx * (Syy * Sz - Sy * Syz) - Sxy * (Sxy * Sz - Sx * Syz) + Sxz * (Sxy * Sy - Syy * Sx)
    Q = D * Szz.astype(object) - Da * Sxz - Db * Syz - Dc * Sz
    return Q, Dc


def classify(columns, step_slabs, robot_slabs, slope, rough):
    """-> namespace: the slope restatement's fields (classes_slope: its classes), and classes int8 [H, W] (-1 unknown, 0 traversable, 100
    BODY, STEP, SLOPE or ROUGH), fit int64 [H, W, 5] (D, Da, Db, Q, n; zeros without a fit), rough (bool), Q, Dc, left, right (object
    arrays of every cell: ROUGH is has_fit and left > right)"""
    num, den = check_rough(rough)
    c = sr.classify(columns, step_slabs, robot_slabs, slope)
    L, K = int(slope[0]), int(slope[1])
    Szz = szz(c.ground, L, K)
    Q, Dc = residual(c.sums, Szz, c.D, c.Da, c.Db)
    left, right = Q * den, c.sums["n"].astype(object) * c.D * num
    is_rough = c.has_fit & (left > right).astype(bool)
    known = c.ground != 255
    fit = np.stack([np.where(c.has_fit, v, 0).astype(np.int64) for v in (c.D, c.Da, c.Db, Q, c.sums["n"].astype(object))], axis=-1)
    classes = np.where(~known, -1, np.where(c.body | c.step | c.slope | is_rough, 100, 0)).astype(np.int8)
    return SimpleNamespace(classes=classes, classes_slope=c.classes, ground=c.ground, fit=fit, body=c.body, step=c.step, has_fit=c.has_fit, slope=c.slope, rough=is_rough,
                           sums=c.sums, szz=Szz, D=c.D, Da=c.Da, Db=c.Db, Dc=Dc, Q=Q, left=left, right=right)


def counts(c, rect=None):
    """(unknown, traversable, BODY, STEP only, SLOPE only, ROUGH only) of a classify() result, of `rect` = (x0, y0, w, h) or the full layer"""
    r = (lambda a: er.restrict(a, rect)) if rect is not None else (lambda a: a)
    classes, body, step, steep, rough = r(c.classes), r(c.body), r(c.step), r(c.slope), r(c.rough)
    return (int((classes == -1).sum()), int((classes == 0).sum()), int(body.sum()), int((step & ~body).sum()), int((steep & ~body & ~step).sum()),
            int((rough & ~body & ~step & ~steep).sum()))


def rough_limit(slab, rms):
    """kicp_elev_rough_limit: (num, den), each operation rounded on its own; None where the entry refuses"""
    with np.errstate(all="ignore"):
        q = np.float64(rms) / np.float64(slab)
        num = np.floor((q * q) * np.float64(1024.0))
    return (int(num), 1024) if np.isfinite(num) and 0 <= num <= 65535 else None


# ---- the fill ---------------------------------------------------------------------------------------------------------------------------
def readout(counts, min_observations):
    """the grid's readout of counters uint16 [..., 2] -> int64: -1 below min_observations, else (100 hits + seen // 2) // seen"""
    hits, misses = counts[..., 0].astype(np.int64), counts[..., 1].astype(np.int64)
    seen = hits + misses
    return np.where((seen < min_observations) | (seen == 0), -1, (100 * hits + seen // 2) // np.maximum(seen, 1))


def fill(dst, src, min_observations, free_max, occupied_min):
    """-> (the destination's counters after the fill, the seven counts)"""
    assert min_observations >= 1 and free_max <= 100 and free_max < occupied_min <= 101 and dst.shape == src.shape
    v = readout(src, min_observations)
    free, occupied = (v >= 0) & (v <= free_max), v >= occupied_min
    obstacle = dst[..., 0] > 0
    unknown = (dst[..., 0] == 0) & (dst[..., 1] == 0)
    traversable = ~obstacle & ~unknown
    out = dst.copy()
    out[unknown & free] = (0, 1)
    out[unknown & occupied] = (1, 0)
    words = (obstacle.sum(), traversable.sum(), (unknown & free).sum(), (unknown & occupied).sum(), (unknown & ~free & ~occupied).sum(), (traversable & occupied).sum(),
             (obstacle & free).sum())
    return out, tuple(int(w) for w in words)
