"""Scenes for the device-side map update (tests/test_gpu_mapdev_regimes.py): pure numpy, seeded, no GPU import.  Each builder returns
world-frame points in INPUT ORDER (the order AddPoints judges them in) plus what makes the scene worth running;
tests/test_mapdev_scenes.py proves that premise on the oracle alone, so that a scene that loses it fails there and not silently on the
GPU."""
import numpy as np

IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def translation(t):
    return np.concatenate([[0.0, 0.0, 0.0, 1.0], np.asarray(t, dtype=np.float64)])


def voxel_keys(pts, vs):
    """PointToVoxel in numpy: the same IEEE division and floor as the reference"""
    return np.floor(np.asarray(pts, dtype=np.float64).reshape(-1, 3) / vs).astype(np.int64)


def map_resolution(vs, cap):
    return np.sqrt(vs * vs / cap)


def in_local_frame(world, t):
    """local points such that local + t (the fp64 sum both the oracle and the kernel form under a pure translation) lies in the voxel
    its world point lies in; returns (local, local + t)"""
    local = np.asarray(world) - np.asarray(t)
    return local, local + np.asarray(t)


# ---- one point per voxel ----------------------------------------------------------------------------------------------
REGION_PITCH = 300.0  # regions lie side by side along x, 300 m apart: further than any range the tests prune with


def region_centre(region):
    return np.array([REGION_PITCH * region + 64.0, 64.0, 0.0])


def one_per_voxel(n, region, extras=1000, cap=20, seed=0):
    """n points, each in a 1 m voxel of its own, on a 128-wide planar grid in region `region` (rows of 128 voxels along x, as many rows as
    n needs).  Then `extras` points within 0.3 map_resolution of an earlier point (the reference drops them) and `extras` more at 1.2 - 1.3
    map_resolution from an earlier point (it keeps them), every one beside a base point of its own and inside that point's voxel.
    -> dict(points (n + 2 extras, 3), n_voxels = n, near / far: index ranges of the two groups)"""
    rng = np.random.default_rng([seed, n, region])
    res = map_resolution(1.0, cap)
    assert 1.3 * res < 0.3 and 2 * extras <= n or extras == 0
    i = np.arange(n)
    corner = np.stack([REGION_PITCH * region + i % 128, i // 128, np.zeros(n)], 1).astype(np.float64)
    base = corner + rng.uniform(0.3, 0.7, (n, 3))
    pick = rng.permutation(n)[:2 * extras]
    d = rng.normal(size=(2 * extras, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    length = np.concatenate([rng.uniform(0.05, 0.3, extras), rng.uniform(1.2, 1.3, extras)]) * res
    pts = np.concatenate([base, base[pick] + d * length[:, None]])
    return dict(points=pts, n_voxels=n, near=slice(n, n + extras), far=slice(n + extras, n + 2 * extras), vs=1.0, cap=cap)


# ---- deep buckets ------------------------------------------------------------------------------------------------------
def deep_voxels(cap, voxels=40, per_voxel=750, seed=0):
    """`voxels` unit voxels 3 m apart (an 8-wide grid around the origin), `per_voxel` offers each: in a voxel's own sequence every even
    offer is uniform in the voxel, every odd one a copy of an earlier offer of the same voxel jittered by sigma = 0.2 map_resolution (kept
    inside the voxel) - so that rejections for closeness happen at every depth of the bucket.  The voxels' sequences are interleaved at
    random in the input order.  -> dict(points, voxel (index of each point's voxel), corners)"""
    rng = np.random.default_rng([seed, cap, voxels, per_voxel])
    res = map_resolution(1.0, cap)
    v = np.arange(voxels)
    corners = np.stack([3.0 * (v % 8) - 12.0, 3.0 * (v // 8) - 6.0, np.zeros(voxels)], 1)
    seq = np.empty((voxels, per_voxel, 3))
    for j in range(per_voxel):
        if j % 2 == 0:
            seq[:, j] = rng.uniform(0.0, 1.0, (voxels, 3))
        else:
            earlier = rng.integers(0, j, voxels)
            seq[:, j] = np.clip(seq[v, earlier] + rng.normal(0.0, 0.2 * res, (voxels, 3)), 0.0, 1.0 - 1e-9)  # (corner + 1 - 1e-9 stays below corner + 1)
    label = rng.permutation(np.repeat(v, per_voxel))
    nth = np.zeros(voxels, dtype=np.int64)
    pts = np.empty((voxels * per_voxel, 3))
    for k, lv in enumerate(label):
        pts[k] = corners[lv] + seq[lv, nth[lv]]
        nth[lv] += 1
    return dict(points=pts, voxel=label, corners=corners, vs=1.0, cap=cap)


def shallow_voxels(n_voxels, centre, per_voxel=3, seed=0):
    """`n_voxels` adjacent unit voxels (a 20-wide grid beside `centre`) with `per_voxel` <= 3 well separated points each, voxel by voxel"""
    rng = np.random.default_rng([seed, n_voxels, per_voxel])
    v = np.arange(n_voxels)
    corner = np.floor(np.asarray(centre, dtype=np.float64)) + np.stack([v % 20 - 10.0, v // 20 - 5.0, np.zeros(n_voxels)], 1)
    spots = np.array([[0.2, 0.2, 0.5], [0.5, 0.7, 0.5], [0.8, 0.3, 0.5]])[:per_voxel]
    pts = corner[:, None, :] + spots[None] + rng.uniform(-0.02, 0.02, (n_voxels, per_voxel, 3))
    return pts.reshape(-1, 3)


# ---- the acceptance radius met exactly ----------------------------------------------------------------------------------
RADIUS_LATTICES = [(1.0, 64), (0.5, 16), (2.0, 4), (1.0, 1)]  # sqrt(vs * vs / cap) is exactly 0.125, 0.125, 1.0, 1.0
# Pairs of one voxel at a distance == map_resolution that the reference must judge, at least (tests/test_mapdev_scenes.py):
#   cap 64 / 16: the scene is built from 3 000 axis neighbours, 7/8 resp. 3/4 of them inside one voxel: 1 000 as the least.
#   cap 4 (8 sites per voxel, the first 4 offered get in): 6 pairs among them, 12 of the cube's 28 pairs are edges -> 2.57 per voxel;
#     +-6 voxels (288 whole voxels) would give 740 +- 21, so this variant spans +-8 voxels: 512 voxels, 1 316 +- 28.
#   cap 1 (one site per voxel): a voxel is full after its first point, the radius is never consulted: 0, whatever the range.  The
#     variant is there for its points on voxel corners and for the `size == cap` test coming first.
RADIUS_MIN_PAIRS = {64: 1000, 16: 1000, 4: 1000, 1: 0}
# voxels either side of the origin in x and y (z: +-1).  The two coarse lattices are wider than +-6 so that they hold the pairs above and
# more than the 4 096 points from which AddPoints goes through the device.
RADIUS_HALF_VOXELS = {64: 6, 16: 6, 4: 8, 1: 20}


def radius_lattice(vs, cap, seed=0):
    """Points on integer multiples of map_resolution over +-6 voxels (RADIUS_HALF_VOXELS: +-8 / +-20 for cap 4 / 1) in x and y and +-1
    voxel in z - every voxel face and the negative side included -, shuffled, a fifth of them repeated as exact duplicates.  The fine lattices (cap 64, 16: too many sites for one
    frame) are sampled as 3 000 sites and, for each, its neighbour one step along a random axis; the coarse ones are taken whole.
    -> dict(points, res)"""
    rng = np.random.default_rng([seed, cap])
    res = map_resolution(vs, cap)
    steps = int(round(vs / res))
    assert res * steps == vs and res in (0.125, 1.0)
    wide = RADIUS_HALF_VOXELS[cap]
    half = np.array([wide * steps, wide * steps, steps])
    if cap >= 16:
        site = rng.integers(-half, half + 1, (3000, 3))
        step = np.zeros((3000, 3), dtype=np.int64)
        step[np.arange(3000), rng.integers(0, 3, 3000)] = rng.choice([-1, 1], 3000)
        ijk = np.concatenate([site, np.clip(site + step, -half, half)])
    else:
        ax = [np.arange(-h, h + 1) for h in half]
        ijk = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    ijk = np.concatenate([ijk, ijk[rng.integers(0, len(ijk), len(ijk) // 5)]])
    pts = rng.permutation(ijk).astype(np.float64) * res  # (exact: res is a power of two)
    return dict(points=pts, res=res, vs=vs, cap=cap)


def division_lattice(vs, cap=20, n=6000, seed=0):
    """Points k * vs for integer k in +-200 per coordinate (z: +-2), vs in {0.1, 0.3}: every point sits on a voxel corner in exact
    arithmetic, and for some k the double k * vs divided by the double vs falls below k - PointToVoxel's division decides the voxel."""
    rng = np.random.default_rng([seed, int(round(vs * 10))])
    k = np.concatenate([rng.integers(-200, 201, (n, 2)), rng.integers(-2, 3, (n, 1))], 1)
    return dict(points=k.astype(np.float64) * vs, k=k, vs=vs, cap=cap)


# ---- the pruning radius met exactly ---------------------------------------------------------------------------------------
def _signs(p):
    """p with every combination of signs of its non-zero coordinates"""
    return [[sx * p[0], sy * p[1], sz * p[2]] for sx in ((1, -1) if p[0] else (1,)) for sy in ((1, -1) if p[1] else (1,))
            for sz in ((1, -1) if p[2] else (1,))]


def prune_edge(max_distance=25.0, filler=4096, seed=0):
    """Voxels (1 m) around the origin whose FIRST point decides whether they survive RemovePointsFarFromLocation(origin = 0):
      exact   first point exactly 25 away - integer triples, every square and sum exact -: removed (`>=`)
      inside  such points moved one np.nextafter towards the origin in every non-zero coordinate: kept
      first_out / first_in   a first point beyond 25 with a later point of the same voxel inside (the whole voxel goes) and the reverse
                             (the whole voxel stays)
    plus `filler` points within 14 m, one per voxel, so that a bulk insertion takes the set.  -> dict(points, keep (bool per point), groups)"""
    assert max_distance == 25.0
    rng = np.random.default_rng([seed, filler])
    exact = np.array(sum([_signs(p) for p in ([15, 20, 0], [7, 24, 0], [12, 16, 15], [9, 12, 20], [0, 25, 0], [0, 15, 20])], []), dtype=np.float64)
    inside = np.array(sum([_signs(p) for p in ([20, 15, 0], [24, 7, 0], [16, 12, 15], [12, 9, 20], [25, 0, 0], [15, 0, 20])], []), dtype=np.float64)
    inside = np.where(inside != 0.0, np.nextafter(inside, 0.0), inside)
    # voxel (17, 18, 0) and its mirror images: near corner 24.76 from the origin, far corner 26.2
    first_out, first_in = [], []
    for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
        first_out += [[sx * 17.9, sy * 18.9, 0.5], [sx * 17.05, sy * 18.05, 0.5]]  # 26.0 then 24.8, one voxel
        first_in += [[sx * 18.05, sy * 17.05, 0.5], [sx * 18.9, sy * 17.9, 0.5]]   # 24.8 then 26.0, one voxel
    first_out, first_in = np.array(first_out), np.array(first_in)
    side = int(np.ceil(filler ** (1 / 3)))  # one point in each voxel of a cube around the origin: nothing is dropped for closeness
    fill = (np.stack(np.meshgrid(*[np.arange(side) - side // 2] * 3, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(0.1, 0.9, (side ** 3, 3)))
    fill, filler = rng.permutation(fill), side ** 3
    groups, pts, keep, at = {}, [], [], 0
    for name, p, k in (("fill_a", fill[:filler // 2], True), ("exact", exact, False), ("inside", inside, True), ("first_out", first_out, False),
                       ("first_in", first_in, True), ("fill_b", fill[filler // 2:], True)):
        groups[name] = slice(at, at + len(p))
        pts.append(p), keep.append(np.full(len(p), k)), (at := at + len(p))
    return dict(points=np.concatenate(pts), keep=np.concatenate(keep), groups=groups, vs=1.0, cap=20, max_distance=max_distance)


# ---- a first update that is "too tight" --------------------------------------------------------------------------------------
START_SLOTS = 1024  # the table a fresh map starts with (kicp_host_map.hpp)


def isolated(n=30, centre=(0.0, 0.0, 0.0), seed=0):
    """n unit voxels at least 3 apart (a 6-wide grid of pitch 3 beside `centre`), one point each.  For a fresh map (1 024 slots, no entry)
    n = 30 is chosen from map_update_device's arithmetic: no re-hash beforehand (2 (0 + 30) <= 1 024), no room for the worst case
    (4 (0 + 27 * 30) = 3 240 > 3 * 1 024 = 3 072: the staged path), and after the claim step - 30 entries, 30 voxels that may become
    occupied - 4 (30 + 26 * 30) = 3 240 > 3 072: too tight, re-hash, claim again.  Isolated voxels make the count exact: no two share a
    neighbour.  Any n from 29 (4 * 27 * 29 = 3 132) to 512 would do."""
    rng = np.random.default_rng([seed, n])
    v = np.arange(n)
    corner = np.floor(np.asarray(centre, dtype=np.float64)) + np.stack([3.0 * (v % 6) - 9.0, 3.0 * (v // 6) - 6.0, np.zeros(n)], 1)
    return corner + rng.uniform(0.2, 0.8, (n, 3))


def too_tight_premise(n, entries=0, slots=START_SLOTS):
    """(no re-hash beforehand, no one-queue head-room, too tight after the claim) by map_update_device's three inequalities"""
    return (entries + n) * 2 <= slots, (entries + 27 * n) * 4 > 3 * slots, (entries + n + 26 * n) * 4 > 3 * slots


# ---- two frames whose cloud comes out in ONE order ---------------------------------------------------------------------------
# Pointcloud() lists the occupied voxels in table order, and a slot is claimed by whichever thread comes first: two maps that took the
# same frames agree on the ORDER of their clouds only where no two voxels claimed in one launch compete for a slot.  The two frames
# below are chosen so (tests/test_mapdev_scenes.py proves it from the table's arithmetic restated here).
ORDERED_FRAMES = ((100, 0), (300, 2))  # (voxels, region) of the first and the second frame, one point per voxel
ORDERED_SLOTS = 32768  # the table after the first frame: too tight in the fresh 1 024 slots, re-hashed for 4 (32 * 100 + 1 024) slots


def ordered_frames():
    """-> the two frames' world points (identity pose; a map with max_distance 1 000 prunes neither)"""
    return [one_per_voxel(n, region, 0)["points"] for n, region in ORDERED_FRAMES]


def voxel_hash(keys):
    """kicp_common.hpp voxel_hash over rows of integer keys"""
    k = np.asarray(keys, dtype=np.int64)
    h = ((k[:, 0] * 73856093) ^ (k[:, 1] * 19349669) ^ (k[:, 2] * 83492791)) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def slots_taken_alone(filled, keys):
    """the slot each key takes by linear probing into `filled` (bool per slot) when it is the only one inserted.  Where these are
    distinct every insertion order gives them: a key's walk only passes slots that were filled before, never another key's"""
    out = []
    for home in voxel_hash(keys) % len(filled):
        s = int(home)
        while filled[s]:
            s = (s + 1) % len(filled)
        out.append(s)
    return np.array(out)


# ---- queries for the final checks ----------------------------------------------------------------------------------------------
def jittered_queries(cloud, vs, n=2000, seed=0):
    """about n queries: points of `cloud` moved by a tenth of a voxel (gaussian), a tenth of them by a voxel or more"""
    rng = np.random.default_rng([seed, len(cloud)])
    if len(cloud) == 0:
        return rng.normal(0, vs, (n, 3))
    q = cloud[rng.integers(0, len(cloud), n)] + rng.normal(0, 0.1 * vs, (n, 3))
    q[::10] += rng.normal(0, 1.0 * vs, (len(q[::10]), 3))
    return q
