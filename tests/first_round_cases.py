"""Scenes for the first visiting round of the one-lane-per-query four-waves pass kernel (kicp_kernels.hpp: gather32_pass's first
round, visit_first, process_trip FRESH), each built so that one regime of that round is provably entered - premises() proves it on the
CPU from the oracle's data and the kernel's arithmetic as tests/test_margin_model.py re-enacts it.  Voxel size 1 m, tau 0.5 m, every
scan registered from the identity, so that the regimes are those of a call's first pass.

  halo    (a) queries whose own voxel holds no points although a neighbour's does (a thin wall just across a voxel face): a whole wave
              of 64 consecutive queries in that state, a wave that mixes both states, at least a quarter of the scan
  across  (b) the nearest point lies in a neighbour although the own voxel holds points, with exact ties across a face (coordinates
              are binary fractions: the two fp64 squared distances are equal) - the earlier shift wins
  deep    (c) max_points_per_voxel = 40: two trips per bucket, the winner in the second one for part of the queries
  beyond  (d) own-voxel candidates on both sides of tau, close enough that the kernel's own-voxel minimum falls in
              (bound_u, bound_u + margin_u] for some; a neighbour's point within tau, or nothing else at all
  mixed   (e) all of the above states and queries without any entry (no point in the 27 voxels), for scans of 1 ... 1 000 points
  near    (f) two and three near-equal candidates in the own voxel: the runner-up within the margin, the third place within it
"""
import numpy as np

from checkers import okicp
from test_margin_model import kernel_key_value

VS, TAU = 1.0, 0.5
UPM = 65536.0 / VS
LENGTHS = (1, 63, 65, 255, 257, 1000)


def search_numbers(tau=TAU, vs=VS):
    """(bound_u, margin_u) of search_params(), units^2, in the kernel's fp32 arithmetic"""
    bound = tau * tau * (1.0 + 9.1e-13)
    bcap = min(bound, 12.0 * vs * vs)
    margin = 2.2 * (5.55e-5 * np.sqrt(bcap) * vs + 4.2e-6 * bcap + 7.7e-10 * vs * vs)
    upm = 65536.0 / vs
    margin_u = np.float32(margin * upm * upm) * np.float32(1.00001)
    bound_u = np.float32(bound * upm * upm) * np.float32(1.00001) + margin_u
    return np.float32(bound_u), np.float32(margin_u)


class Scene:
    def __init__(self, cap):
        self.cap = cap
        self.map_points = []   # in insertion order
        self.frames = {}       # name -> (n, 3) queries
        self.tags = {}         # name -> per-query tag (what the query was built to be)

    def add_map(self, pts):
        self.map_points.extend(np.asarray(pts, dtype=np.float64).reshape(-1, 3))

    def finish(self):
        self.map_points = np.array(self.map_points)
        self.frames = {k: np.ascontiguousarray(np.array(v, dtype=np.float64).reshape(-1, 3)) for k, v in self.frames.items()}
        self.tags = {k: np.array(v) for k, v in self.tags.items()}
        return self


def _cells(n, base, per_row=10, pitch=3):
    """origins (integer voxel corners) of n isolated cells, three voxels apart: a cell's points and its query's 27 voxels span
    -1 .. 1, so no cell sees another's points"""
    return [np.array(base, dtype=np.float64) + pitch * np.array([i % per_row, i // per_row, 0.0]) for i in range(n)]


def build():
    rng = np.random.default_rng(41)
    s = Scene(20)
    # ---- (a) a thin wall in the voxels x = 10, queries just across the face x = 10 (voxels x = 9: empty) and inside the wall ----
    side = 12
    for j in range(side):
        for k in range(side):
            s.add_map([[10.05, j + 0.2 + 0.5 * a, k + 0.2 + 0.5 * b] for a in (0, 1) for b in (0, 1)])
    n_halo_scan = 1500
    state = np.concatenate([np.ones(64, bool), np.arange(64) % 2 == 0, rng.random(n_halo_scan - 128) < 0.4])  # True: across the face
    yz = rng.uniform(0.0, side, (n_halo_scan, 2))
    x = np.where(state, rng.uniform(9.72, 9.9, n_halo_scan), rng.uniform(10.1, 10.4, n_halo_scan))
    s.frames["halo"] = np.column_stack([x, yz])
    s.tags["halo"] = np.where(state, "empty_own", "inside")
    # ---- (b) nearest point across a face, exact ties (binary fractions) -------------------------------------------------------
    # (query, own-voxel points, neighbour points), local to the cell's voxel corner
    across = {
        "tie_own_-x": ((0.125, 0.5, 0.5), [(0.375, 0.5, 0.5)], [(-0.125, 0.5, 0.5)]),
        "tie_own_-z": ((0.5, 0.5, 0.125), [(0.5, 0.5, 0.375)], [(0.5, 0.5, -0.125)]),
        "tie_own_y_-x": ((0.125, 0.25, 0.5), [(0.125, 0.5, 0.5)], [(-0.125, 0.25, 0.5)]),
        "tie_-x_-y": ((0.25, 0.25, 0.5), [(0.25, 0.25, 0.9375)], [(-0.125, 0.25, 0.5), (0.25, -0.125, 0.5)]),
        "tie_+x_+y": ((0.75, 0.75, 0.5), [(0.75, 0.75, 0.0625)], [(0.75, 1.125, 0.5), (1.125, 0.75, 0.5)]),
        "nearer_-x": ((0.125, 0.5, 0.5), [(0.5, 0.5, 0.5)], [(-0.125, 0.5, 0.5)]),
        "nearer_+y_+z": ((0.5, 0.875, 0.875), [(0.5, 0.5, 0.5)], [(0.5, 1.0625, 1.0625)]),
    }
    names = list(across)
    s.frames["across"], s.tags["across"] = [], []
    for c, origin in enumerate(_cells(70 * 4, (24.0, 0.0, 20.0), per_row=20)):
        name = names[c % len(names)]
        q, own, nb = across[name]
        jitter = np.array([0.0, 0.0, 0.0]) if "y" in name or "z" in name else np.array([0.0, (c // 7 % 8) / 64.0, (c // 56 % 8) / 64.0])
        pts = [np.array(p) + jitter + origin for p in own + nb]
        order = rng.permutation(len(pts))  # (whichever voxel is filled first: the visiting order decides, not the insertion order)
        s.add_map([pts[o] for o in order])
        s.frames["across"].append(np.array(q) + jitter + origin)
        s.tags["across"].append(name)
    # ---- (d) own-voxel candidates on both sides of tau ------------------------------------------------------------------------
    s.frames["beyond"], s.tags["beyond"] = [], []
    distances = [0.45, 0.4999, 0.50003, 0.50006, 0.50008, 0.5001, 0.50012, 0.5002, 0.52]
    for c, origin in enumerate(_cells(len(distances) * 2 * 16, (24.0, 0.0, -30.0), per_row=18)):
        d = distances[c % len(distances)]
        with_neighbour = (c // len(distances)) % 2 == 1
        q = origin + np.array([0.125, 0.3, 0.3]) + np.concatenate([[0.0], rng.uniform(0.0, 0.4, 2)])
        s.add_map([q + [d, 0.0, 0.0]])
        if with_neighbour:
            s.add_map([q - [0.375, 0.0, 0.0]])
        s.frames["beyond"].append(q)
        s.tags["beyond"].append(("in" if d < TAU else "out") + ("+neighbour" if with_neighbour else ""))
    # ---- (f) two and three near-equal candidates in the own voxel -------------------------------------------------------------
    s.frames["near"], s.tags["near"] = [], []
    eps = [0.0, 1e-7, -1e-7, -2e-5, 6e-5, 4e-4]  # (0.6 eps m^2 between the squared distances; the margin is 6.3e-5 m^2)
    for c, origin in enumerate(_cells(len(eps) * len(eps) * 2 * 3, (24.0, 0.0, 40.0), per_row=18)):
        e1, e2 = eps[c % len(eps)], eps[(c // len(eps)) % len(eps)]
        three = (c // (len(eps) * len(eps))) % 2 == 1
        q = origin + rng.uniform(0.45, 0.55, 3)
        pts = [q + [0.3, 0.0, 0.0], q + [0.0, 0.3 + e1, 0.0]] + ([q - [0.0, 0.0, 0.3 + e2]] if three else [])
        s.add_map([pts[o] for o in rng.permutation(len(pts))])
        s.frames["near"].append(q)
        s.tags["near"].append("three" if three else "two")
    s.finish()
    # ---- (e) every state in one scan, and queries with no entry at all --------------------------------------------------------
    nothing = np.column_stack([rng.uniform(0, 30, 120), rng.uniform(0, 30, 120), np.full(120, -70.0)])
    parts = [("halo", s.frames["halo"][64:700]), ("across", s.frames["across"][:120]), ("beyond", s.frames["beyond"][:120]),
             ("near", s.frames["near"][:60]), ("no_entry", nothing)]
    mixed = np.concatenate([p for _, p in parts])
    tags = np.concatenate([np.full(len(p), t) for t, p in parts])
    order = rng.permutation(len(mixed))
    s.frames["mixed"], s.tags["mixed"] = np.ascontiguousarray(mixed[order]), tags[order]
    return s


def build_deep():
    """(c) buckets of forty points: a slab of full voxels, the insertion order of each voxel's points shuffled"""
    rng = np.random.default_rng(43)
    s = Scene(40)
    lattice = np.array([[0.125 + 0.25 * i, 0.125 + 0.25 * j, 0.125 + 0.25 * k] for i in range(4) for j in range(4) for k in range(3)])
    for vx in range(6):
        for vy in range(6):
            pick = rng.permutation(len(lattice))[:40]
            s.add_map(lattice[pick] + rng.uniform(-0.02, 0.02, (40, 3)) + [vx, vy, 0.0])
    n = 1200
    s.frames["deep"] = np.column_stack([rng.uniform(0.0, 6.0, (n, 2)), rng.uniform(0.0, 0.8, n)])
    s.tags["deep"] = np.full(n, "deep")
    return s.finish()


def oracle_map(scene):
    m = okicp.VoxelHashMap(VS, 100.0, scene.cap)
    m.AddPoints(scene.map_points)
    assert m.num_points() == len(scene.map_points)  # (every point was kept: a voxel's bucket order is the insertion order)
    return m


def _voxels(p):
    return np.floor(np.asarray(p) / VS).astype(np.int64)


def _occupied(scene):
    return {tuple(v) for v in _voxels(scene.map_points)}


def own_voxel_states(scene, frame):
    """per query: (own voxel holds points, some of the 26 neighbours does)"""
    occ = _occupied(scene)
    shifts = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    v = _voxels(frame)
    own = np.array([tuple(x) in occ for x in v])
    nb = np.array([any((x[0] + a, x[1] + b, x[2] + c) in occ for a, b, c in shifts) for x in v])
    return own, nb


def own_voxel_keys(scene, frame):
    """per query: the kernel's keys (units^2, ascending) of the points of its own voxel"""
    vox = _voxels(scene.map_points)
    index = {}
    for i, v in enumerate(map(tuple, vox)):
        index.setdefault(v, []).append(i)
    out = []
    for q in frame:
        members = index.get(tuple(_voxels(q)), [])
        if not members:
            out.append(np.zeros(0))
            continue
        p = scene.map_points[members]
        out.append(np.sort(kernel_key_value(np.repeat(q[None], len(p), 0), p, VS) * (UPM * UPM)))
    return out


def premises(scene, omap):
    """assert that every regime a scene was built for is entered; returns the counts for the record"""
    I = okicp.IDENTITY
    bound_u, margin_u = search_numbers()
    seen = {}
    if "halo" in scene.frames:
        f = scene.frames["halo"]
        own, nb = own_voxel_states(scene, f)
        empty_own = ~own & nb
        assert np.array_equal(empty_own, scene.tags["halo"] == "empty_own")
        assert empty_own.mean() >= 0.25 and empty_own[:64].all() and 8 < empty_own[64:128].sum() < 56
        acc, _, _ = okicp.associate(omap, f, I, TAU)
        assert acc[empty_own].mean() > 0.5 and acc[~empty_own].mean() > 0.5  # (both states do find correspondences)
        seen["halo"] = (int(empty_own.sum()), len(f))
    if "across" in scene.frames:
        f, tags = scene.frames["across"], scene.tags["across"]
        own, nb = own_voxel_states(scene, f)
        assert own.all() and nb.all()
        acc, nn, d = okicp.associate(omap, f, I, TAU)
        assert acc.all()
        left = np.any(_voxels(nn) != _voxels(f), axis=1)  # the pick lies in a neighbour voxel
        ties = 0
        for i, (q, t) in enumerate(zip(f, tags)):
            d2 = np.sort(np.sum((scene.map_points - q) ** 2, axis=1))
            if t.startswith("tie"):
                assert d2[0] == d2[1] < d2[2]  # exactly equidistant in fp64
                ties += 1
                assert left[i] == (not t.startswith("tie_own"))  # the own voxel is the first shift of the order
            else:
                assert d2[0] < d2[1] and left[i]
        # (between two neighbours the earlier shift of the reference's order wins: +x before +y, -x before -y)
        for t, axis in (("tie_-x_-y", 0), ("tie_+x_+y", 0)):
            k = tags == t
            assert np.all(_voxels(nn[k])[:, axis] != _voxels(f[k])[:, axis])
        seen["across"] = (ties, int(left.sum()), len(f))
    if "beyond" in scene.frames:
        f, tags = scene.frames["beyond"], scene.tags["beyond"]
        acc, nn, d = okicp.associate(omap, f, I, TAU)
        left = np.any(_voxels(nn) != _voxels(f), axis=1)
        assert not acc[tags == "out"].any() and acc[tags == "in"].all() and not left[tags == "in"].any()
        assert acc[tags == "out+neighbour"].all() and left[tags == "out+neighbour"].all()
        m1 = np.array([k[0] for k in own_voxel_keys(scene, f)], dtype=np.float32)
        below, gate, above = m1 <= bound_u, (m1 > bound_u) & (m1 <= bound_u + margin_u), m1 > bound_u + margin_u
        out = np.char.startswith(tags, "out")
        assert (gate & out).sum() >= 16 and (above & out).sum() >= 16 and (below & out).sum() >= 16 and (below & ~out).sum() >= 16
        seen["beyond"] = (int((below & out).sum()), int((gate & out).sum()), int((above & out).sum()), len(f))
    if "near" in scene.frames:
        f, tags = scene.frames["near"], scene.tags["near"]
        keys = own_voxel_keys(scene, f)
        two = np.array([k[1] - k[0] <= margin_u for k in keys])
        three = np.array([len(k) > 2 and k[2] - k[0] <= margin_u for k in keys])
        assert (two & (tags == "two")).sum() >= 30 and (~two & (tags == "two")).sum() >= 8
        assert (three & (tags == "three")).sum() >= 30 and (two & ~three & (tags == "three")).sum() >= 8
        assert okicp.associate(omap, f, I, TAU)[0].all()
        seen["near"] = (int(two.sum()), int(three.sum()), len(f))
    if "mixed" in scene.frames:
        f, tags = scene.frames["mixed"], scene.tags["mixed"]
        assert len(f) >= max(LENGTHS)
        own, nb = own_voxel_states(scene, f)
        assert not (own | nb)[tags == "no_entry"].any() and (tags[:63] == "no_entry").any() and (~own & nb)[:63].any() and own[:63].any()
        assert not okicp.associate(omap, f[tags == "no_entry"], I, TAU)[0].any()
        seen["mixed"] = (int((tags == "no_entry").sum()), int((~own & nb).sum()), len(f))
    if "deep" in scene.frames:
        f = scene.frames["deep"]
        acc, nn, d = okicp.associate(omap, f, I, TAU)
        assert acc.all()
        # position of the pick inside its voxel's bucket = its rank among that voxel's points in insertion order
        vox = _voxels(scene.map_points)
        rank = {}
        count = {}
        for p, v in zip(map(tuple, scene.map_points), map(tuple, vox)):
            rank[p] = count.get(v, 0)
            count[v] = rank[p] + 1
        assert set(count.values()) == {40}
        pos = np.array([rank[tuple(p)] for p in nn])
        assert (pos >= 20).mean() > 0.25 and (pos < 20).mean() > 0.25
        seen["deep"] = (int((pos >= 20).sum()), len(f))
    return seen
