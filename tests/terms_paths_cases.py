"""Scenes for the two paths of the pass kernels' limb split (kicp_pass_fixed.hpp::terms_to_fixed): the short one where all five terms of a
correspondence are below 2^22 in magnitude, to_fixed's where one is not.  A term that large is s.x^2 + s.y^2 of a source point more than
2 048 m from the base frame, so the far queries sit at about 3 000 m.

Every coordinate is a multiple of 1/64 below 4 096 and the pose is a translation by such numbers: all products are multiples of 2^-12
below 2^24, every term is exact in fp64, a sum of a few hundred of them is exact in fp64 whatever the order, and a term is a multiple
of the kernel's 2^-40 grid.  So the oracle's sums carry no rounding of their own and the kernel's must equal them BIT FOR BIT - a limb
dropped or doubled on either path, or a lane sent down the wrong one, shows in the last bit.  (A rotated pose has no such property; the
GPU test holds its builds to one another there.)

The map: 256 points in 24 voxels at x = 3 000 (a grid of 2 x 64 x 2, 3/8 m apart along y) and 8 points in one voxel at the origin - 25
voxels.  Query i is map point `target[i]` plus an offset of its own of at most 3/64 m per axis: nearer to it than to anything else (the
grid's spacing is 3/8 m), inside TAU.  premises() proves on the CPU, with the oracle, what a scene claims."""
from dataclasses import dataclass

import numpy as np

from checkers import okicp

VS, CAP, MAX_DISTANCE, TAU = 1.0, 20, 1.0e4, 0.25
POSE = np.array([0.0, 0.0, 0.0, 1.0, 8.0, -4.0, 0.0])  # a translation: T s = s + t, exactly
SHORT_LIMIT = 4194304.0  # 2^22 (kShortTermLimit)


def map_points():
    far = np.array([[3000.0 + x, 0.125 + 0.375 * k, z] for k in range(64) for x in (0.125, 0.5) for z in (0.125, 0.5)])
    near = np.array([[x, y, z] for x in (0.125, 0.5) for y in (0.125, 0.5) for z in (0.125, 0.5)])
    return far, near


def offsets(n):
    """n offsets, multiples of 1/64 in [-3/64, 3/64]^3 (5 and 343 are coprime: distinct for n <= 343)"""
    grid = np.array([[a, b, c] for a in range(-3, 4) for b in range(-3, 4) for c in range(-3, 4)], dtype=np.float64) / 64.0
    return grid[(np.arange(n) * 5) % len(grid)]


@dataclass
class Scene:
    name: str
    n: int
    far: np.ndarray      # bool[n]: the query's correspondence has s.x^2 + s.y^2 >= 2^22
    queries: np.ndarray  # source points, base frame
    images: np.ndarray   # T * queries
    target: np.ndarray   # the map point each query was built beside
    tiles: int = 0       # "pass_tiles" of the four-waves build (0: the automatic rule)


def _scene(name, n, far_mask, tiles=0):
    far_pts, near_pts = map_points()
    far_mask = np.asarray(far_mask, dtype=bool)
    target = np.where(far_mask[:, None], far_pts[np.arange(n) % len(far_pts)], near_pts[np.arange(n) % len(near_pts)])
    images = target + offsets(n)
    return Scene(name, n, far_mask, images - POSE[4:], images, target, tiles)


def one_lane():
    return _scene("one_lane", 256, np.arange(256) == 5)


def spread_64():
    """64 far queries, sixteen in every wave"""
    return _scene("spread_64", 256, np.arange(256) % 4 == 1)


def whole_wave():
    """every lane of wave 0, none of the other waves"""
    return _scene("whole_wave", 256, np.arange(256) < 64)


def every_lane():
    return _scene("every_lane", 256, np.ones(256, dtype=bool))


def no_lane():
    return _scene("no_lane", 256, np.zeros(256, dtype=bool))


def two_tiles():
    """two blocks of one workgroup: the first all near, every other query of the second far"""
    i = np.arange(512)
    return _scene("two_tiles", 512, (i >= 256) & (i % 2 == 0), tiles=2)


BUILDERS = {f.__name__: f for f in (one_lane, spread_64, whole_wave, every_lane, no_lane, two_tiles)}


def oracle_map():
    far, near = map_points()
    omap = okicp.VoxelHashMap(VS, MAX_DISTANCE, CAP)
    omap.AddPoints(np.concatenate([far, near]))
    return omap


def terms_of(scene):
    """the five terms per query as correspondence_terms forms them at POSE (R = 1: c0 = UnitX, c1 = UnitY), exact in fp64 here"""
    s, r = scene.queries, scene.images - scene.target
    return np.stack([-s[:, 1], s[:, 0] ** 2 + s[:, 1] ** 2, r[:, 0], s[:, 0] * r[:, 1] - s[:, 1] * r[:, 0], (r ** 2).sum(1)], axis=1)


def exact_sums(scene):
    """[JTJ00, JTJ01, JTJ11, JTr0, JTr1, ssq, N] from integers: every term times 2^12 is an integer below 2^36"""
    t = terms_of(scene) * 4096.0
    assert np.array_equal(t, np.rint(t)) and np.abs(t).max() < 2.0 ** 36
    col = [int(v) for v in t.astype(np.int64).sum(0)]
    return np.array([float(scene.n), col[0] / 4096.0, col[1] / 4096.0, col[2] / 4096.0, col[3] / 4096.0, col[4] / 4096.0, float(scene.n)])


def premises(scene, omap):
    """what the scene claims, by the oracle: returns the number of far queries"""
    far, near = map_points()
    assert omap.num_points() == len(far) + len(near) and omap.num_voxels() <= 27 and scene.n <= 512
    q64 = np.concatenate([scene.queries, scene.images, scene.target]) * 64.0
    assert np.array_equal(q64, np.rint(q64)) and np.abs(q64).max() < 64.0 * 4096.0  # multiples of 1/64 below 4 096
    assert np.array_equal(scene.queries + POSE[4:], scene.images)  # (the pose acts exactly)
    acc, nn, d = okicp.associate(omap, scene.queries, POSE, TAU)
    assert acc.all() and np.array_equal(nn, scene.target) and d.max() < TAU  # every query: its own map point, accepted
    t = np.abs(terms_of(scene))
    large = (t >= SHORT_LIMIT).any(1)
    assert np.array_equal(large, scene.far)                  # exactly the far queries leave the short path ...
    assert np.array_equal(t[:, 1] >= SHORT_LIMIT, scene.far)  # ... through s.x^2 + s.y^2 ...
    assert t.max() < 2.0 ** 43                                # ... and none leaves the accumulation's range
    if scene.far.any() and not scene.far.all():
        waves = scene.far.reshape(-1, 64)
        assert (waves.any(1) & ~waves.all(1)).any() or (waves.all(1).any() and (~waves.any(1)).any())  # waves that diverge, or that differ
    return int(scene.far.sum())
