"""Scenes for the second word of a mirror point (kicp_common.hpp::MirrorPoint: z as the float the pass kernels subtract the query from,
an empty slot as 4 294 901 760.0f), the smallest at which that word can go wrong - each a handful of 1 m voxels and at most 512 queries,
registered from the identity with tau 0.5 m.  premises() proves on the CPU, from the oracle's picks and a model of the buckets, that every
regime a scene was built for is entered.

A scene is a list of steps, so that a test can build its map twice - on the host and through UpdateDevice - and look at it between
steps:
    ("update", points, origin)   AddPoints(points), then RemovePointsFarFromLocation(origin)
    ("sweep",)                   RemoveSeenThrough of the wall view (tests/view_cases.py)
Every map coordinate is a binary fraction and every origin an integer vector, so that (p - origin) + origin == p exactly: the device
route (a frame at the pose `origin`) files the very same doubles as the host route.

  fills     max_points_per_voxel 20: buckets of 1, 19 and 20 points.  Empty slots must lose; the full bucket's trip ends at the stride -
            the bucket filed right behind it holds points exactly where the full voxel's queries are, as seen from their voxels' corners
  trips21   max_points_per_voxel 21 (a stride of two trips): buckets of 20 (the first trip's last slot occupied, the second trip
            empty), and of 21 points (the second trip holds one point - the nearest one for some queries)
  trips40   max_points_per_voxel 40: buckets of 20, 21 and 40 points, picks in the first and the last slot of the second trip
  (all)     points ON the z faces of their voxel: mirror z exactly 0 (the word 0x00000000 must still count as a point - also in the last
            slot of a first trip, where it decides whether the bucket goes on) and exactly 65 535; queries whose nearest neighbour is
            such a point, from the own voxel and from the voxel across that face (an empty own voxel whose only occupied neighbour
            holds one point)
  reuse     a full bucket emptied by RemovePointsFarFromLocation and handed to a new voxel that holds two points: the eighteen slots
            behind them held points before, exactly where the new voxel's queries are
  swept     the same through the map sweep on the device (view_cases' wall and its "full_bucket_erased" map) and an update after it
"""
import numpy as np

from checkers import okicp
from test_margin_model import mirror_quant

VS, TAU = 1.0, 0.5
UPM = 65536.0 / VS
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
ZERO = np.zeros(3)
TOP = 1.0 - 2.0 ** -20  # an offset just inside the far face: rounds to 65 536 units, clamped to 65 535
LENGTHS = (1, 63, 65, 257)  # scans that end inside a wave

# offsets inside a voxel 0.25 apart: any two of them are farther apart than the map's resolution at 20, 21 and 40 points per voxel
# (0.224, 0.218 and 0.158 m), so AddPoints accepts every one
LATTICE = np.array([[0.125 + 0.25 * i, 0.125 + 0.25 * j, 0.125 + 0.25 * k] for k in range(4) for j in range(4) for i in range(4)])


class Model:
    """the map's buckets as AddPoints / RemovePointsFarFromLocation / the sweep leave them: voxel -> its points in bucket order"""

    def __init__(self, cap, max_distance):
        self.cap, self.max_distance, self.buckets = cap, max_distance, {}

    def add(self, pts):
        res = np.sqrt(VS * VS / self.cap)
        for p in np.asarray(pts, dtype=np.float64).reshape(-1, 3):
            b = self.buckets.setdefault(tuple(np.floor(p / VS).astype(int)), [])
            assert len(b) < self.cap and all(np.linalg.norm(p - o) >= res for o in b), "the scene offers a point the map would refuse"
            b.append(p.copy())

    def remove_far(self, origin):
        for v in [v for v, b in self.buckets.items() if np.linalg.norm(b[0] - origin) >= self.max_distance]:
            del self.buckets[v]

    def keep_only(self, cloud):
        left = {tuple(p) for p in cloud}
        for v in list(self.buckets):
            self.buckets[v] = [p for p in self.buckets[v] if tuple(p) in left]
            if not self.buckets[v]:
                del self.buckets[v]

    def points(self):
        return np.array([p for b in self.buckets.values() for p in b]).reshape(-1, 3)

    def rank(self):
        """point -> its position in its bucket"""
        return {tuple(p): k for b in self.buckets.values() for k, p in enumerate(b)}

    def count(self, p):
        return len(self.buckets[tuple(np.floor(np.asarray(p) / VS).astype(int))])


class Scene:
    def __init__(self, name, cap, max_distance=50.0):
        self.name, self.cap, self.max_distance = name, cap, max_distance
        self.steps = []     # see the module's docstring
        self.looks = {}     # number of steps done -> name of the state to test there
        self.queries = {}   # state -> (n, 3)
        self.marks = {}     # state -> {what: indices of the queries built for it}


def _near(points, k, rng):
    """a query at most 0.05 m from points[k], in the same voxel: that point is its nearest neighbour by a wide margin"""
    d = rng.uniform(0.01, 0.03, 3)
    if points[k][2] - np.floor(points[k][2]) > 0.9:
        d[2] = -d[2]
    return points[k] + d


def _cell_queries(origin, pts, rng, marks, tag, ranks):
    """queries next to the points at `ranks` of a bucket, a query from across the nearest face for each, and a few anywhere around"""
    out = []
    for r in ranks:
        marks.setdefault("%s_rank%d" % (tag, r), []).append(len(marks["_all"]) + len(out))
        out.append(_near(pts, r, rng))
        # from the neighbour voxel across the face nearest to that point (0.125 m away on a lattice point's low side)
        off = pts[r] - origin
        axis = int(np.argmin(np.minimum(off, 1.0 - off)))
        if len(pts) > 1 and min(off[axis], 1.0 - off[axis]) > 0.2:
            continue  # (a point in the middle of a shared voxel: a query across the face could be nearer to another one)
        step = np.zeros(3)
        step[axis] = -(off[axis] + 0.07) if off[axis] < 0.5 else (1.0 - off[axis]) + 0.07
        marks.setdefault("%s_rank%d_across" % (tag, r), []).append(len(marks["_all"]) + len(out))
        out.append(pts[r] + step)
    out.extend(origin + rng.uniform(-0.45, 1.45, (6, 3)))
    marks["_all"].extend(out)


def _bucket(origin, n, rng, z0_at=None, top_at=None):
    """n points of one voxel on the lattice, shuffled; position z0_at lies ON the near z face (mirror z 0, and x = y = 0 too where the
    position is 0: the whole slot is zero), position top_at just inside the far z face (mirror z 65 535)"""
    inner = LATTICE[(LATTICE[:, 2] > 0.3) & (LATTICE[:, 2] < 0.7)]  # (the z-face points keep their distance from these)
    pick = inner[rng.permutation(len(inner))] if (z0_at is not None or top_at is not None) else LATTICE[rng.permutation(len(LATTICE))]
    assert n <= len(pick)
    pts = pick[:n].copy()
    if z0_at is not None:
        pts[z0_at] = [0.0, 0.0, 0.0] if z0_at == 0 else [0.5, 0.5, 0.0]
    if top_at is not None:
        pts[top_at] = [0.5, 0.25, TOP]
    return pts + origin


def _fill_scene(name, cap, cells, seed):
    """cells: (tag, origin, n, z0_at, top_at, ranks to aim queries at); one update files them all in this order"""
    rng = np.random.default_rng(seed)
    s = Scene(name, cap)
    marks = {"_all": []}
    cloud = []
    for tag, origin, n, z0_at, top_at, ranks in cells:
        origin = np.array(origin, dtype=np.float64)
        pts = _bucket(origin, n, rng, z0_at, top_at)
        cloud.append(pts)
        _cell_queries(origin, pts, rng, marks, tag, ranks)
    s.steps.append(("update", np.concatenate(cloud), ZERO))
    # queries without any entry: nothing in their 27 voxels
    marks["no_entry"] = list(range(len(marks["_all"]), len(marks["_all"]) + 5))
    marks["_all"].extend(np.array([30.5, 30.5, 5.5]) + rng.uniform(-0.4, 0.4, (5, 3)))
    q = np.array(marks.pop("_all"))
    order = rng.permutation(len(q))  # (neighbouring lanes belong to different cells)
    inverse = np.argsort(order)
    s.queries["built"] = np.ascontiguousarray(q[order])
    s.marks["built"] = {k: inverse[np.array(v)] for k, v in marks.items()}
    s.looks[1] = "built"
    return s


def fills():
    cells = [("one", (0, 0, 0), 1, None, None, [0]),
             ("nineteen", (3, 0, 0), 19, None, None, [0, 18]),
             ("twenty", (6, 0, 0), 20, None, None, [0, 19]),
             ("decoy", (9, 0, 0), 20, None, None, [0]),
             ("z0_alone", (0, 3, 0), 1, 0, None, [0]),
             ("top_alone", (3, 3, 0), 1, None, 0, [0]),
             ("z0_last", (6, 3, 0), 20, 19, None, [19, 5]),
             ("top_last", (9, 3, 0), 20, None, 19, [19, 5]),
             ("z0_mid", (0, 6, 0), 7, 3, 6, [3, 6])]
    s = _fill_scene("fills", 20, cells, 11)
    # the trap behind the full bucket: "decoy" is filed right after "twenty"; queries into "twenty" that sit exactly where the decoy's
    # points are, as seen from their voxels' corners - a trip that ran past the stride would find them at distance zero
    pts = s.steps[0][1]
    twenty, decoy = pts[20:40], pts[40:60]
    assert np.all(np.floor(twenty[:, 0]) == 6) and np.all(np.floor(decoy[:, 0]) == 9)
    trap = decoy - [3.0, 0.0, 0.0]
    n = len(s.queries["built"])
    s.queries["built"] = np.ascontiguousarray(np.concatenate([s.queries["built"], trap]))
    s.marks["built"]["trap"] = np.arange(n, n + len(trap))
    return s


def trips21():
    cells = [("twenty", (0, 0, 0), 20, None, None, [0, 19]),
             ("twentyone", (3, 0, 0), 21, None, None, [0, 19, 20]),
             ("z0_last_of_trip", (6, 0, 0), 21, 19, 20, [19, 20]),
             ("top_last_of_trip", (9, 0, 0), 21, 20, 19, [19, 20]),
             ("one", (0, 3, 0), 1, None, None, [0])]
    return _fill_scene("trips21", 21, cells, 12)


def trips40():
    cells = [("twenty", (0, 0, 0), 20, None, None, [0, 19]),
             ("twentyone", (3, 0, 0), 21, None, None, [19, 20]),
             ("forty", (6, 0, 0), 40, None, None, [0, 19, 20, 39]),
             ("z0_first_of_trip", (9, 0, 0), 24, 20, 19, [19, 20, 23]),
             ("decoy", (0, 3, 0), 40, None, None, [39])]
    return _fill_scene("trips40", 40, cells, 13)


def reuse():
    """a bucket emptied and re-used on the host's terms (RemovePointsFarFromLocation)"""
    rng = np.random.default_rng(14)
    s = Scene("reuse", 20)
    stale = LATTICE[rng.permutation(len(LATTICE))]
    stay = _bucket(np.array([0.0, 0.0, 0.0]), 12, rng)
    doomed = stale[:20] + [72.0, 0.0, 0.0]   # 42 m from the first origin, 72 m from the second
    s.steps.append(("update", np.concatenate([stay, doomed]), np.array([30.0, 0.0, 0.0])))
    s.looks[1] = "before"
    s.steps.append(("update", np.array([[3.5, 0.5, 0.5]]), ZERO))           # the doomed voxel goes: its bucket is free, its words stay
    fresh = stale[20:22] + [6.0, 0.0, 0.0]                                  # the next new voxel takes the freed bucket: two points
    s.steps.append(("update", fresh, ZERO))
    s.looks[3] = "after"
    around = np.concatenate([stay[:6] + rng.uniform(-0.03, 0.03, (6, 3)), rng.uniform(-0.4, 1.4, (12, 3))])
    s.queries["before"] = np.ascontiguousarray(np.concatenate([around, doomed[:8] + rng.uniform(-0.03, 0.03, (8, 3))]))
    s.marks["before"] = {"doomed": np.arange(len(around), len(around) + 8)}
    # where the freed bucket's old points are, as seen from the new voxel's corner: slots 2 .. 19 must read empty
    ghosts = stale[2:20] + [6.0, 0.0, 0.0]
    s.queries["after"] = np.ascontiguousarray(np.concatenate([around, ghosts, fresh + 0.02]))
    s.marks["after"] = {"ghosts": np.arange(len(around), len(around) + len(ghosts)), "fresh": np.arange(len(around) + len(ghosts), len(around) + len(ghosts) + 2)}
    return s


def swept():
    """a bucket emptied by the map sweep on the device and re-used by the update behind it"""
    import view_cases as vc
    rng = np.random.default_rng(15)
    case = vc.sweep_cases()["full_bucket_erased"]
    assert case["vs"] == VS and case["cap"] == 20
    s = Scene("swept", 20, max_distance=100.0)
    s.steps.append(("update", case["points"], ZERO))
    s.looks[1] = "before"
    s.steps.append(("sweep",))
    s.looks[2] = "swept"
    gone = case["points"][:20]  # voxel (10, 0, 0), all twenty seen through
    fresh = np.array([[10.625, 0.375, 0.375], [10.625, 0.75, 0.75]])  # the same voxel again, behind the line the wall draws: two points
    s.steps.append(("update", fresh, ZERO))
    s.looks[3] = "after"
    around = np.concatenate([case["points"][20:33] + rng.uniform(-0.03, 0.03, (13, 3)), np.array([10.0, 0.0, 0.0]) + rng.uniform(-0.4, 1.4, (12, 3))])
    at_gone = gone + rng.uniform(-0.01, 0.01, (20, 3))
    for state in ("before", "swept", "after"):
        s.queries[state] = np.ascontiguousarray(np.concatenate([around, at_gone] + ([fresh - 0.02] if state == "after" else [])))
        s.marks[state] = {"gone": np.arange(len(around), len(around) + 20)}
    s.marks["after"]["fresh"] = np.arange(len(around) + 20, len(around) + 22)
    return s


BUILDERS = {"fills": fills, "trips21": trips21, "trips40": trips40, "reuse": reuse, "swept": swept}


def wall_render():
    """the wall frame's image by the restatement: (frame, depth, sensor position, render statistics)"""
    import view_cases as vc
    import view_ref as vr
    frame = vc.wall()
    depth, stats, c = vr.render(vc.WALL_CFG, frame, vc.IDENTITY, vc.ORIGIN)
    return frame, depth, c, stats


def replay(scene, wall=None):
    """the scene's states on the CPU: state name -> (Model at that moment (a snapshot of its buckets), oracle map holding those buckets)"""
    from mapdev_ref import bucket_sorted
    model = Model(scene.cap, scene.max_distance)
    states = {}
    for k, step in enumerate(scene.steps):
        if step[0] == "update":
            model.add(step[1])
            model.remove_far(step[2])
        else:
            import view_cases as vc
            import view_ref as vr
            _, depth, c, _ = wall
            before = bucket_sorted(model.points(), VS)
            keep, stats = vr.sweep(vc.WALL_CFG, depth, c, before, VS)
            assert stats[3] >= 1  # a voxel is erased
            model.keep_only(before[keep])
        if k + 1 in scene.looks:
            snap = Model(scene.cap, scene.max_distance)
            snap.buckets = {v: list(b) for v, b in model.buckets.items()}
            omap = okicp.VoxelHashMap(VS, scene.max_distance, scene.cap)
            omap.AddPoints(snap.points())
            assert omap.num_points() == len(snap.points())
            states[scene.looks[k + 1]] = (snap, omap)
    return states


def expected(scene, states, state):
    """the oracle on a state's queries: (accepted, targets, distances, rank of each accepted target in its bucket)"""
    snap, omap = states[state]
    q = scene.queries[state]
    acc, nn, d = okicp.associate(omap, q, IDENTITY, TAU)
    rank = snap.rank()
    return acc, nn, d, np.array([rank[tuple(p)] if a else -1 for p, a in zip(nn, acc)])


def _qz(p):
    return mirror_quant(p[2] - np.floor(p[2] / VS) * VS, UPM)


def premises(scene, states):
    """assert that the regimes the scene was built for are entered; returns counts for the record"""
    seen = {}
    assert all(len(q) <= 512 for q in scene.queries.values())
    if scene.name in ("fills", "trips21", "trips40"):
        snap, omap = states["built"]
        acc, nn, d, rank = expected(scene, states, "built")
        marks = scene.marks["built"]
        q = scene.queries["built"]
        own = np.array([tuple(np.floor(x / VS).astype(int)) in snap.buckets for x in q])
        assert not acc[marks["no_entry"]].any()
        for what, idx in marks.items():
            if "_rank" not in what:
                continue
            want = int(what.split("_rank")[1].split("_")[0])
            assert acc[idx].all() and np.all(rank[idx] == want), what  # the pick is the point in that slot ...
            assert own[idx].all() != what.endswith("_across"), what    # ... from its own voxel, or from the empty voxel across the face
        counts = sorted({snap.count(p) for p in nn[acc]})
        seen["bucket sizes picked from"] = counts
        qz = np.array([_qz(p) for p in nn[acc]])
        seen["picks with mirror z 0 / 65535"] = (int((qz == 0).sum()), int((qz == 65535).sum()))
        assert (qz == 0).sum() >= 2 and (qz == 65535).sum() >= 2
        if scene.name == "fills":
            assert counts == [1, 7, 19, 20]
            # an empty own voxel whose only occupied neighbour holds one point, and that point on a z face
            for what in ("one_rank0_across", "z0_alone_rank0_across", "top_alone_rank0_across"):
                i = marks[what]
                assert acc[i].all() and not own[i].any() and all(snap.count(p) == 1 for p in nn[i])
            assert all(_qz(p) == 0 for p in nn[marks["z0_alone_rank0"]]) and all(_qz(p) == 65535 for p in nn[marks["top_alone_rank0"]])
            # the word 0x00000000 in a trip's last slot: the bucket is full, the slot holds a point (the pick)
            assert all(_qz(p) == 0 and np.all(p[:2] - np.floor(p[:2]) == 0.5) for p in nn[marks["z0_last_rank19"]])
            assert np.all(nn[marks["z0_alone_rank0"]] == [0.0, 3.0, 0.0])  # x = y = z = 0: both words of the slot are zero
            # the trap: the oracle picks inside "twenty" (or nothing), never the decoy
            t = marks["trap"]
            assert acc[t].sum() >= 10 and np.all(np.floor(nn[t][acc[t]][:, 0]) == 6)
            seen["trap"] = int(acc[t].sum())
        else:
            assert 20 in counts and 21 in counts and (scene.name == "trips21" or 40 in counts)
            assert (rank >= 20).sum() >= 4 and (rank == 19).sum() >= 4
            if scene.name == "trips40":
                assert (rank == 39).sum() >= 2
            seen["picks in the second trip"] = int((rank >= 20).sum())
    elif scene.name == "reuse":
        acc, nn, d, rank = expected(scene, states, "before")
        m = scene.marks["before"]["doomed"]
        assert acc[m].all() and np.all(np.floor(nn[m][:, 0]) == 72)
        snap, _ = states["after"]
        assert (72, 0, 0) not in snap.buckets and len(snap.buckets[(6, 0, 0)]) == 2
        acc, nn, d, rank = expected(scene, states, "after")
        g = scene.marks["after"]["ghosts"]
        assert len(g) == 18 and 2 <= acc[g].sum() < 18 and np.all(rank[g][acc[g]] < 2) and acc[scene.marks["after"]["fresh"]].all()
        seen["ghost queries that find one of the two real points"] = int(acc[g].sum())
    elif scene.name == "swept":
        snap, _ = states["swept"]
        assert (10, 0, 0) not in snap.buckets and (10, 0, 0) in states["before"][0].buckets and len(states["after"][0].buckets[(10, 0, 0)]) == 2
        acc, nn, d, rank = expected(scene, states, "before")
        g = scene.marks["before"]["gone"]
        assert acc[g].all() and np.all(np.floor(nn[g]) == [10, 0, 0])
        acc, nn, d, rank = expected(scene, states, "swept")
        assert not np.any(np.all(np.floor(nn[acc]) == [10, 0, 0], axis=1))
        acc, nn, d, rank = expected(scene, states, "after")
        own = np.all(np.floor(nn) == [10, 0, 0], axis=1) & acc
        assert own[scene.marks["after"]["fresh"]].all() and np.all(rank[own] < 2)
        seen["queries at the removed points that find something else"] = int(acc[g].sum())
    return seen
