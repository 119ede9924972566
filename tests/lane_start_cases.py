"""Scenes for the start of a lane and the set-up of a visit in the pass kernels (kicp_pass_visit.hpp: voxel_coord's constant guard, the
lane offsets taken from its fraction, query_from for each of the 27 shifts, the lending round), each built so that one regime is provably
entered - premises() proves it on the CPU from the oracle's data.  Every map fills at most the 27 voxels of one block; a scan is one or
two blocks of 256 queries (1, 255, 256, 257 and 512 queries).

  shifts       one query per shift of the reference's order whose accepted neighbour lies in that very voxel: every one of the shifts
               decides a result (voxels on both sides of 0)
  negative     the same with every coordinate below 0
  faces        query coordinates exactly on voxel faces (0.0, positive and negative integers; one, and all three axes): the fraction is
               0 and the division decides
  guard        coordinates 2^-20 voxel sizes (9.5e-7) above and below a face, on every axis: inside the constant guard of 1e-6, far
               outside the guard relative to |t| it replaced - the division decides where the fast path used to be trusted
  guard_tenth  voxel size 0.1: z coordinates where floor(c (1 / vs)) is NOT floor(c / vs) (0.3 and -0.7000000000000001), the target two
               voxels from the voxel the fast path names - without the guard the search looks in the wrong neighbourhood
  lend         every wave of 64 queries holds lanes with three or more voxels still alive after the first round and lanes with none:
               from round 2 the first kind lends two voxels each to the second (gather32_pass, one lane per query)
  single       one query

Queries come in pairs mirrored through their common target (q, 2 p - q), padded with queries that sit on a map point, and every
coordinate that enters a term is a binary fraction of at most 20 bits behind the point: the sums of J^T r are exact and exactly 0 in the
reference's doubles and in the kernels' fixed point alike, so the registration from the identity ends after ONE iteration at the
identity, bit for bit - unless a correspondence is wrong.  (guard_tenth keeps x and y binary; z enters no term of J^T r.)"""
import numpy as np

from checkers import okicp
from first_round_cases import search_numbers

I = okicp.IDENTITY
# the reference's visiting order (kiss-icp v1.2.0 core/VoxelHashMap.cpp voxel_shifts; kicp_common.hpp::kShiftTable)
SHIFTS = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0),
                   (1, 0, 1), (1, 0, -1), (-1, 0, 1), (-1, 0, -1), (0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1), (1, 1, 1), (1, 1, -1),
                   (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1)], dtype=np.float64)
EPS = 2.0 ** -20       # of a voxel: inside the constant guard
GUARD = 1.0e-6         # kicp_pass_visit.hpp::kVoxelGuard


class Scene:
    def __init__(self, name, n, vs=1.0, tau=0.5, seed=7):
        self.name, self.n, self.vs, self.tau, self.cap = name, n, vs, tau, 20
        self.map_points, self._pairs, self._tags = [], [], []
        self._rng = np.random.default_rng(seed)

    def block(self, corner):
        """one point in each of the 27 voxels around the voxel at `corner`: p_s = corner + 0.5 + 0.625 shift_s"""
        self.corner = np.array(corner, dtype=np.float64)
        self.map_points = list(self.corner + 0.5 + 0.625 * SHIFTS)

    def pair(self, q, p, tag):
        """a query, and its mirror image through the target"""
        q, p = np.array(q, dtype=np.float64), np.array(p, dtype=np.float64)
        self._pairs += [q, 2.0 * p - q]
        self._tags += [tag, "twin"]

    def finish(self, twins_keep_z=False):
        self.map_points = np.array(self.map_points)
        q, tags = list(self._pairs), list(self._tags)
        if twins_keep_z:
            for k in range(1, len(q), 2):
                q[k][2] = q[k - 1][2]
        assert len(q) <= self.n
        for k in range(self.n - len(q)):  # queries on a map point: no residual, nothing alive after the first round
            q.append(self.map_points[k % len(self.map_points)].copy())
            tags.append("pad")
        order = self._rng.permutation(len(q))
        self.queries = np.ascontiguousarray(np.array(q)[order])
        self.tags = np.array(tags)[order]
        return self


def _shift_queries(s, corner):
    s.block(corner)
    s.pair(s.corner + 0.5 + [0.125, 0.0, 0.0], s.corner + 0.5, "shift_0")
    for k in range(1, 27):
        s.pair(s.corner + 0.5 + 0.375 * SHIFTS[k], s.corner + 0.5 + 0.625 * SHIFTS[k], "shift_%d" % k)


def build_shifts():
    s = Scene("shifts", 257)
    _shift_queries(s, (3, -1, 0))
    return s.finish()


def build_negative():
    s = Scene("negative", 255)
    _shift_queries(s, (-3, -3, -3))
    return s.finish()


def build_lend():
    s = Scene("lend", 512, seed=11)
    for _ in range(3):
        _shift_queries(s, (0, 0, 0))
    return s.finish()


def build_single():
    s = Scene("single", 1)
    s.block((1, 1, 1))
    s._pairs, s._tags = [s.corner + [0.5, 0.5, 0.875]], ["shift_5"]  # (its residual lies along z: no term of J^T r sees it)
    return s.finish()


def build_faces():
    s = Scene("faces", 256)
    s.block((0, -1, -2))
    c = s.corner
    for axis in range(3):
        for side in (0.0, 1.0):  # the face towards the lower neighbour (the voxel is the block's centre), and towards the upper one
            q = c + 0.5
            q[axis] = c[axis] + side
            p = q.copy()
            p[axis] += 0.125 if side else -0.125
            s.pair(q, p, "face_%d_%d" % (axis, int(side)))
    s.pair(c + 1.0, c + 1.125, "face_all_1")
    s.pair(c, c - 0.125, "face_all_0")
    return s.finish()


def build_guard():
    s = Scene("guard", 257)
    s.block((-1, 0, 2))
    c = s.corner
    for axis in range(3):
        for side, name in ((EPS, "low"), (1.0 - EPS, "high")):
            q = c + 0.5
            q[axis] = c[axis] + side
            p = c + 0.5
            p[axis] = c[axis] + (1.125 if name == "high" else -0.125)
            s.pair(q, p, "guard_%d_%s" % (axis, name))
    s.pair(c + [EPS, 1.0 - EPS, EPS], c + [-0.125, 1.125, -0.125], "guard_all")
    return s.finish()


TENTH = {"up": 0.3, "down": -0.7000000000000001}  # floor(c * 10.0): 3 and -8; floor(c / 0.1): 2 and -7


def build_guard_tenth():
    s = Scene("guard_tenth", 255, vs=0.1, tau=0.15)
    s.corner = np.zeros(3)
    x, y, r = 3.0 / 64.0, 3.0 / 64.0, 1.0 / 64.0
    s.map_points = [np.array([x + r, y, 0.19]), np.array([x - r, y + 0.125, -0.59])]  # in voxels z = 1 and z = -6
    s.pair([x, y, TENTH["up"]], s.map_points[0], "tenth_up")
    s.pair([x, y + 0.125, TENTH["down"]], s.map_points[1], "tenth_down")
    return s.finish(twins_keep_z=True)


BUILDERS = {"shifts": build_shifts, "negative": build_negative, "faces": build_faces, "guard": build_guard, "guard_tenth": build_guard_tenth,
            "lend": build_lend, "single": build_single}


def oracle_map(scene):
    m = okicp.VoxelHashMap(scene.vs, 100.0, scene.cap)
    m.AddPoints(scene.map_points)
    assert m.num_points() == len(scene.map_points)
    return m


def _voxels(p, vs):
    return np.floor(np.asarray(p) / vs).astype(np.int64)  # (the reference's PointToVoxel)


def _fractions(c, vs):
    """t = c (1 / vs), its fraction, the guard relative to |t| of the formula before - in the kernel's arithmetic"""
    t = np.asarray(c) * (1.0 / vs)
    return t, t - np.floor(t), 4.0e-16 * np.abs(t) + 1.0e-300


def _alive_after_round_one(scene, q):
    """(voxels surely alive, voxels possibly alive) of query q after a first round at its own voxel: cull_todo's test, lower bound <=
    (best + 4 margin) 1.00001, with 2 % to either side for the fp32 arithmetic"""
    vs = scene.vs
    upm2 = (65536.0 / vs) ** 2
    bound_u, margin_u = search_numbers(scene.tau, vs)
    occupied = {tuple(v) for v in _voxels(scene.map_points, vs)}
    own = _voxels(q, vs)
    assert tuple(own) in occupied  # (so the first round visits the own voxel)
    mine = scene.map_points[np.all(_voxels(scene.map_points, vs) == own, axis=1)]
    best = min(float(np.min(np.sum((mine - q) ** 2, axis=1))), float(bound_u) / upm2)
    surely = possibly = 0
    for shift in SHIFTS[1:]:
        if tuple(own + shift.astype(np.int64)) not in occupied:
            continue
        lb = sum(((own[a] + 1) * vs - q[a]) ** 2 if shift[a] > 0 else (q[a] - own[a] * vs) ** 2 for a in range(3) if shift[a] != 0)
        surely += lb <= 0.98 * best
        possibly += lb <= 1.02 * (best + 4.0 * float(margin_u) / upm2)
    return surely, possibly


def premises(scene, omap):
    """assert that the scene enters the regime it was built for; returns what it counted"""
    vs, q, tags = scene.vs, scene.queries, scene.tags
    assert len(q) == scene.n and len({tuple(v) for v in _voxels(scene.map_points, vs)}) <= 27
    acc, nn, d = okicp.associate(omap, q, I, scene.tau)
    assert acc.all()
    # J^T r of the first pass at the identity: every term a multiple of 2^-40 (the kernels' fixed point holds it unrounded), both sums 0
    r = q - nn
    terms = np.column_stack([r[:, 0], -q[:, 1] * r[:, 0] + q[:, 0] * r[:, 1]])
    scaled = terms * 2.0 ** 40
    assert np.array_equal(scaled, np.round(scaled)) and np.abs(scaled).max() < 2.0 ** 52
    if scene.n > 1:
        assert terms[:, 0].sum() == 0.0 and terms[:, 1].sum() == 0.0 and np.abs(terms).sum() > 0.0
    else:
        assert not terms.any() and r[0, 2] != 0.0
    seen = {"n": scene.n}
    went = _voxels(nn, vs) - _voxels(q, vs)
    if scene.name in ("shifts", "negative", "lend"):
        for k in range(27):
            rows = np.flatnonzero(tags == "shift_%d" % k)
            assert len(rows) >= 1 and np.all(went[rows] == SHIFTS[k].astype(np.int64)) and np.all(d[rows] > 0.0)
        seen["shifts"] = 27
    if scene.name == "negative":
        assert np.all(q < 0.0)
    if scene.name == "shifts":
        assert (q < 0.0).any() and (q > 0.0).any()
    if scene.name == "single":
        assert tuple(went[0]) == (0, 0, 1)
    if scene.name == "faces":
        rows = np.flatnonzero(np.char.startswith(tags, "face_"))
        t, frac, _ = _fractions(q[rows], vs)
        on_face = frac == 0.0
        assert np.array_equal(on_face.sum(axis=1), np.where(np.char.startswith(tags[rows], "face_all"), 3, 1)) and len(rows) == 8
        values = set(t[on_face])
        assert 0.0 in values and min(values) < 0.0 < max(values)
        assert np.any(went[rows] != 0, axis=1).sum() >= 4  # (the lower faces: the neighbour holds the target)
        seen["faces"] = int(on_face.sum())
    if scene.name == "guard":
        rows = np.flatnonzero(np.char.startswith(tags, "guard_"))
        t, frac, old = _fractions(q[rows], vs)
        new_only = (np.abs(frac - 0.5) > 0.5 - GUARD) & ~((frac < old) | (1.0 - frac < old))
        low, high = new_only & (frac < 0.5), new_only & (frac > 0.5)
        assert np.array_equal(new_only.sum(axis=1), np.where(tags[rows] == "guard_all", 3, 1)) and len(rows) == 7
        assert low.any(axis=0).all() and high.any(axis=0).all() and (t[new_only] < 0.0).any()  # both sides on every axis
        assert np.any(went[rows] != 0, axis=1).all()
        seen["guard"] = (int(low.sum()), int(high.sum()))
    if scene.name == "guard_tenth":
        for tag, c in (("tenth_up", TENTH["up"]), ("tenth_down", TENTH["down"])):
            row = np.flatnonzero(tags == tag)
            assert len(row) == 1 and q[row[0], 2] == c
            fast, exact = int(np.floor(c * (1.0 / vs))), int(np.floor(c / vs))
            assert abs(fast - exact) == 1 and _voxels(q[row[0]], vs)[2] == exact
            t, frac, old = _fractions(c, vs)
            assert frac < old or 1.0 - frac < old  # (the guard it replaced caught it too)
            assert abs(_voxels(nn[row[0]], vs)[2] - fast) == 2  # out of the wrong voxel's reach
        seen["guard_tenth"] = 2
    if scene.name == "lend":
        waves = []
        for w in range(0, scene.n, 64):
            alive = [_alive_after_round_one(scene, x) for x in q[w:w + 64]]
            rich, idle = sum(a[0] >= 3 for a in alive), sum(a[1] == 0 for a in alive)
            assert rich >= 2 and idle >= 2 * 2
            waves.append((rich, idle))
        seen["lend"] = waves
    return seen
