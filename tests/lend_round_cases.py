"""Scenes for the lending round of the one-lane-per-query pass kernels (kicp_kernels.hpp::gather32_pass): from the second visiting round on,
lanes with no voxel left take over voxels of lanes that have more than one.  One wave of 64 queries per scene (256 for the job cap), all
in the voxel [0, 1)^3, at most four map points in at most four voxels:

    M3 = the centre of the own voxel, of +x (shift 1) and of +y (shift 3): (0.5, 0.5, 0.5), (1.125, 0.5, 0.5), (0.5, 1.125, 0.5)
    M4 = M3 and the centre of ++0 (shift 7): (1.125, 1.125, 0.5)

and five kinds of query (z jittered by multiples of 2^-11 so that no two of a wave are equal; no voxel above or below holds points):

    pad      on the own voxel's point: distance 0, nothing alive after the first round - an idle lane
    one      (0.95, 0.5):   only +x alive, which holds its neighbour - a busy lane with nothing to spare
    two_*    +x and +y alive: the lane visits +x itself and has +y to give away
               two_nothing  (0.95, 0.8):  +x holds the neighbour, +y nothing within tau
               two_win      (0.8, 0.95):  +x holds nothing within tau, +y the neighbour: the LENT visit finds the winner
               two_tie      (0.95, 0.95): the points of +x and +y are at the same distance to the last bit; the reference keeps the first
                                          in visiting order, +x - the owner's own candidate must survive the merge of the lent one
    three    (0.95, 0.95) on M4: +x, +y and ++0 alive, two voxels to give away; +y holds a candidate within tau that loses, ++0, the
             last of them, the neighbour

premises() replays the first lending round on the CPU (which lanes are busy, idle, how many voxels each can spare, how the jobs are dealt)
from the voxels cull_todo leaves alive after the first round, and asserts what each scene claims."""
import numpy as np

from checkers import okicp
from first_round_cases import search_numbers
from lane_start_cases import SHIFTS

I = okicp.IDENTITY
VS, TAU, CAP = 1.0, 0.5, 20
LEND_JOBS = 32  # kLendJobs
OWN, PX, PY, PXY = (0.5, 0.5, 0.5), (1.125, 0.5, 0.5), (0.5, 1.125, 0.5), (1.125, 1.125, 0.5)
M3, M4 = np.array([OWN, PX, PY]), np.array([OWN, PX, PY, PXY])
KINDS = {"pad": (0.5, 0.5), "one": (0.95, 0.5), "two_nothing": (0.95, 0.8), "two_win": (0.8, 0.95), "two_tie": (0.95, 0.95), "three": (0.95, 0.95)}


class Scene:
    def __init__(self, name, map_points, counts, waves=1, seed=5):
        """counts: {kind: queries per wave}; the kinds are shuffled inside every wave"""
        assert sum(counts.values()) == 64
        self.name, self.map_points, self.n, self.tau, self.cap = name, map_points, 64 * waves, TAU, CAP
        rng = np.random.default_rng(seed)
        q, kinds = [], []
        for w in range(waves):
            names = [k for k, c in counts.items() for _ in range(c)]
            for j, pos in enumerate(rng.permutation(64)):
                names_at = names[pos]
                x, y = KINDS[names_at]
                z = 0.5 if names_at == "pad" and j % 2 else 0.5 + (1 + j) / 2048.0
                q.append((x, y, z)), kinds.append(names_at)
        self.queries, self.kinds = np.array(q), np.array(kinds)


def no_idle():
    return Scene("no_idle", M4, {"three": 32, "one": 32})


def one_idle_two_voxels():
    return Scene("one_idle_two_voxels", M4, {"pad": 1, "three": 1, "one": 62})


def more_jobs_than_idle():
    return Scene("more_jobs_than_idle", M4, {"three": 24, "pad": 8, "one": 32})


def more_than_32_jobs():
    return Scene("more_than_32_jobs", M4, {"three": 20, "pad": 44}, waves=4)


def lent_finds_nothing():
    return Scene("lent_finds_nothing", M3, {"two_nothing": 16, "pad": 48})


def lent_finds_winner():
    return Scene("lent_finds_winner", M3, {"two_win": 16, "pad": 48})


def lent_ties():
    return Scene("lent_ties", M3, {"two_tie": 16, "pad": 48})


BUILDERS = {f.__name__: f for f in (no_idle, one_idle_two_voxels, more_jobs_than_idle, more_than_32_jobs, lent_finds_nothing, lent_finds_winner, lent_ties)}


def oracle_map(scene):
    m = okicp.VoxelHashMap(VS, 100.0, CAP)
    m.AddPoints(scene.map_points)
    assert m.num_points() == len(scene.map_points)
    return m


def alive_after_round_one(scene, q):
    """the shifts (ascending = visiting order) cull_todo leaves alive for query q after a first round at its own voxel: lower bound <=
    (best + 4 margin) 1.00001.  Asserts that the decision is the same with 2 % to either side (the fp32 arithmetic cannot flip it)."""
    upm2 = 65536.0 ** 2
    bound_u, margin_u = search_numbers(TAU, VS)
    best = min(float(np.sum((np.array(OWN) - q) ** 2)), float(bound_u) / upm2)
    alive = []
    for s in range(1, 27):
        shift = SHIFTS[s]
        if not any(np.array_equal(np.floor(p), shift) for p in scene.map_points):
            continue
        lb = sum((1.0 - q[a]) ** 2 if shift[a] > 0 else q[a] ** 2 for a in range(3) if shift[a] != 0)
        surely, possibly = lb <= 0.98 * best, lb <= 1.02 * (best + 4.0 * float(margin_u) / upm2)
        assert surely == possibly, (scene.name, q, s)
        if surely:
            alive.append(s)
    return alive


def premises(scene, omap):
    """replay round 2 of every wave; returns {"waves": [(busy, idle, jobs offered, jobs lent)], "lent": {nothing, winner, tie, loser}}"""
    q = scene.queries
    assert len(q) == scene.n and len(scene.map_points) <= 27
    for w in range(0, scene.n, 64):  # (no two queries of a wave are equal, the pads on the point itself aside)
        rows = q[w:w + 64][q[w:w + 64, 2] != 0.5]
        assert len({tuple(x) for x in rows}) == len(rows)
    assert np.all(np.floor(q) == 0.0)  # every query's own voxel holds points: the first round visits it
    acc, nn, d = okicp.associate(omap, q, I, TAU)
    assert acc.all()
    seen = {"waves": [], "lent": {"nothing": 0, "winner": 0, "tie": 0, "loser": 0}}
    for w in range(0, scene.n, 64):
        alive = [alive_after_round_one(scene, x) for x in q[w:w + 64]]
        busy = [len(a) > 0 for a in alive]
        spare = [min(2, max(0, len(a) - 1)) for a in alive]
        jobs = [(lane, s) for lane, a in enumerate(alive) for s in a[1:1 + spare[lane]]]  # dealt in lane order, a lane's jobs together
        idle = 64 - sum(busy)
        pairs = min(len(jobs), idle, LEND_JOBS) if jobs and idle else 0
        seen["waves"].append((sum(busy), idle, len(jobs), pairs))
        for lane, s in jobs[:pairs]:
            x, target = q[w + lane], scene.map_points[[np.array_equal(np.floor(p), SHIFTS[s]) for p in scene.map_points]][0]
            dist = np.sqrt(np.sum((target - x) ** 2))
            own_s = alive[lane][0]
            own_target = scene.map_points[[np.array_equal(np.floor(p), SHIFTS[own_s]) for p in scene.map_points]][0]
            if not dist < TAU:
                seen["lent"]["nothing"] += 1
            elif np.array_equal(target, nn[w + lane]):
                seen["lent"]["winner"] += 1
            elif dist == d[w + lane] and np.array_equal(own_target, nn[w + lane]) and own_s < s:
                seen["lent"]["tie"] += 1  # the same distance to the last bit; the oracle kept the owner's, earlier in the order
            else:
                assert dist > d[w + lane]
                seen["lent"]["loser"] += 1  # a candidate within tau that another voxel's beats
    kinds = scene.kinds
    went = {k: {tuple(np.floor(x)) for x in nn[kinds == k]} for k in set(kinds)}
    for k, want in (("pad", (0, 0, 0)), ("one", (1, 0, 0)), ("two_nothing", (1, 0, 0)), ("two_win", (0, 1, 0)), ("two_tie", (1, 0, 0)), ("three", (1, 1, 0))):
        assert went.get(k, {want}) == {want}, (k, went[k])
    return seen
