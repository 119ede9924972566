"""The scenes of tests/mapdev_scenes.py through the oracle alone (okicp, and the reference build where oracle/_ref exists): each
test asserts the premise that makes its scene worth running on the GPU - which offers the reference drops and why, how deep the
buckets get, that a distance really equals the radius.  No GPU."""
import numpy as np
import pytest

import mapdev_scenes as sc
from conftest import sort_rows
from mapdev_ref import Oracles, bucket_sorted


@pytest.mark.parametrize("n,extras", [(8192, 1000), (8193, 1000), (12288, 1000), (14384, 1000), (16384, 0), (16385, 0)])
def test_one_per_voxel(n, extras):
    for region in (0, 2, 1):  # the three regions the GPU tests update one after the other
        s = sc.one_per_voxel(n, region=region, extras=extras)
        pts = s["points"]
        assert len(pts) == n + 2 * extras
        local, world = sc.in_local_frame(pts, sc.region_centre(region))  # what an update at the region's centre inserts
        for p in (pts, world):
            keys = sc.voxel_keys(p, 1.0)
            assert len(np.unique(keys, axis=0)) == len(np.unique(keys[:n], axis=0)) == n == s["n_voxels"]
        # all of it within the tests' range of 150 from the region's centre, the neighbouring regions beyond it
        assert np.linalg.norm(local, axis=1).max() < 100.0
        assert np.linalg.norm(pts - sc.region_centre(region + 1), axis=1).min() > 150.0
    o = Oracles(1.0, 1e6, s["cap"])
    o.AddPoints(pts[:n])
    assert o.num_voxels() == o.num_points() == n
    kept = o.verdicts(pts[n:])
    assert not kept[:extras].any() and kept[extras:].all()
    assert o.num_voxels() == n and o.num_points() == n + extras


@pytest.mark.parametrize("cap", [64, 65, 128, 255])
def test_deep_voxels(cap):
    s = sc.deep_voxels(cap)
    pts, label = s["points"], s["voxel"]
    keys = sc.voxel_keys(pts, 1.0)
    np.testing.assert_array_equal(keys, s["corners"][label].astype(np.int64))  # 40 voxels, the jitter left none of them
    first = np.bincount(label[:24000], minlength=40)
    assert first.min() > 500 and first.max() < 700  # "groups of about 600" in the first update of 24 000
    o = Oracles(1.0, 30.0, cap)
    kept = o.verdicts(pts)
    held = np.zeros(40, dtype=np.int64)  # points in each voxel when the offer arrives
    deep_rejections = offers_after_full = deep_rejections_second = 0
    for i, (v, k) in enumerate(zip(label, kept)):
        if held[v] == cap:
            assert not k
            offers_after_full += 1
        elif not k and held[v] > 64:  # not full, so the radius decided
            deep_rejections += 1
            deep_rejections_second += i >= 24000
        held[v] += k
    assert held.max() == cap and offers_after_full >= 1  # a voxel reaches the cap and is offered more
    # What "deeper than 64" can mean depends on the cap: with 64 no bucket passes 64 (the one-trip edge of the lane-strided loops); with 65
    # a bucket holds more than 64 only when it is full, so the radius is never consulted there (the edge of the second trip); from 66 on
    # offers are judged by distance against more than 64 points.
    if cap > 64:
        assert (held > 64).sum() >= 30
    if cap > 65:
        assert deep_rejections >= 1
    if cap == 255:  # (with 128 every bucket is full after the first 24 000 offers: the second update only finds full, deep buckets)
        assert deep_rejections_second >= 1  # the second update judges by distance against old buckets deeper than 64
    assert o.num_points() == held.sum()


def test_deep_voxels_cap_255_fills_from_300_uniform_offers():
    rng = np.random.default_rng(1)
    o = Oracles(1.0, 1e6, 255)
    o.AddPoints(rng.uniform(0, 1, (300, 3)))
    assert o.num_voxels() == 1 and o.num_points() == 255


@pytest.mark.parametrize("vs,cap", sc.RADIUS_LATTICES)
def test_radius_lattice(vs, cap):
    s = sc.radius_lattice(vs, cap)
    pts, res = s["points"], s["res"]
    assert np.sqrt(vs * vs / cap) == res and res in (0.125, 1.0)
    assert len(pts) <= 16384  # frame-sized
    wide = sc.RADIUS_HALF_VOXELS[cap]
    assert cap >= 16 or len(pts) >= 4096  # (the coarse lattices, taken whole: a bulk AddPoints goes through the device)
    np.testing.assert_array_equal(pts / res, np.round(pts / res))
    keys = sc.voxel_keys(pts, vs)
    assert keys.min(0).tolist() == [-wide, -wide, -1] and keys.max(0).tolist() == [wide, wide, 1]  # negative side, and the far faces' own voxels
    assert (pts == np.floor(pts / vs) * vs).all(1).any()  # points on voxel corners
    for t in (np.zeros(3), np.array([3, -5, 1]) * res):
        o = Oracles(vs, 1e6, cap)
        world = pts + t
        keys = sc.voxel_keys(world, vs)
        kept = o.verdicts(world)
        # replay: per voxel the points kept so far; an offer is JUDGED when its voxel is not full
        held, pairs, judged_at_radius_dropped = {}, 0, 0
        for p, k, key in zip(world, kept, map(tuple, keys)):
            h = held.setdefault(key, [])
            if len(h) < cap:
                d = np.sqrt(((np.array(h).reshape(-1, 3) - p) ** 2).sum(1)) if h else np.zeros(0)
                at_radius = int((d == res).sum())
                pairs += at_radius
                if not k:
                    assert (d < res).any()  # only an exact duplicate (or nothing) lies closer than the radius on this lattice
                    assert (d == 0.0).any()
                if at_radius and not (d < res).any():
                    assert k, "a point exactly map_resolution from its nearest neighbour must be accepted"
            else:
                assert not k
            if k:
                h.append(p)
        assert pairs >= sc.RADIUS_MIN_PAIRS[cap], pairs
        assert o.num_voxels() == len(held)


@pytest.mark.parametrize("vs", [0.1, 0.3])
def test_division_lattice(vs):
    s = sc.division_lattice(vs)
    pts, k = s["points"], s["k"]
    kk = np.arange(-200, 201)
    assert (np.floor((kk * vs) / vs) != kk).any()  # k * vs / vs falls below k for some k: the division decides
    keys = sc.voxel_keys(pts, vs)
    assert (keys != k).any()  # ... and the scene holds such points
    for t in (np.zeros(3), np.array([3, -5, 1]) * vs):
        world = pts + t
        o = Oracles(vs, 1e6, s["cap"])
        o.AddPoints(world)
        wkeys = sc.voxel_keys(world, vs)
        assert o.num_voxels() == len(np.unique(wkeys, axis=0))  # numpy's voxel is the oracle's
        b = o.buckets()
        np.testing.assert_array_equal(np.unique(sc.voxel_keys(b, vs), axis=0), np.unique(wkeys, axis=0))


def test_prune_edge():
    s = sc.prune_edge()
    pts, keep, g = s["points"], s["keep"], s["groups"]
    assert len(pts) >= 4096  # a bulk insertion takes it
    assert np.all((pts[g["exact"]] ** 2).sum(1) == 625.0) and np.all((pts[g["inside"]] ** 2).sum(1) < 625.0)
    keys = sc.voxel_keys(pts, 1.0)
    special = np.concatenate([keys[g[n]] for n in ("exact", "inside", "first_out", "first_in")])
    assert len(np.unique(special, axis=0)) == len(pts[g["exact"]]) + len(pts[g["inside"]]) + 4 + 4  # no two groups share a voxel
    for way in ("update", "add_then_remove"):
        o = Oracles(1.0, s["max_distance"], s["cap"])
        if way == "update":
            o.Update(pts, sc.IDENTITY)
        else:
            o.AddPoints(pts)
            assert o.num_points() == len(pts)  # nothing is dropped for closeness: what goes, goes by the pruning rule
            o.RemovePointsFarFromLocation(np.zeros(3))
        cloud = o.o.Pointcloud()
        np.testing.assert_array_equal(sort_rows(cloud), sort_rows(pts[keep]))
    d = np.linalg.norm(pts, axis=1)
    fo, fi = pts[g["first_out"]], pts[g["first_in"]]
    assert np.all(np.linalg.norm(fo[0::2], axis=1) > 25.5) and np.all(np.linalg.norm(fo[1::2], axis=1) < 25.0)
    assert np.all(np.linalg.norm(fi[0::2], axis=1) < 25.0) and np.all(np.linalg.norm(fi[1::2], axis=1) > 25.5)
    assert d[g["fill_a"]].max() < 14.0 and d[g["fill_b"]].max() < 14.0


def test_isolated():
    pts = sc.isolated(30)
    keys = sc.voxel_keys(pts, 1.0)
    assert len(np.unique(keys, axis=0)) == 30
    diff = np.abs(keys[:, None] - keys[None]).max(2) + 1000 * np.eye(30, dtype=np.int64)
    assert diff.min() >= 3  # no two voxels share a neighbour: 27 entries each
    assert sc.too_tight_premise(30) == (True, True, True)
    # the second update of the same size, elsewhere, into the re-hashed table (1024 * 8 slots hold 4 (0 + 32 * 30 + 1024) = 7 936): room for the worst case
    assert (27 * 30 + 27 * 30) * 4 <= 3 * 8192
    o = Oracles(1.0, 1e6, 20)
    o.AddPoints(pts)
    assert o.num_voxels() == o.num_points() == 30


def test_shallow_voxels_and_queries():
    pts = sc.shallow_voxels(200, (100.0, 0.0, 0.0))
    o = Oracles(1.0, 30.0, 255)
    local, world = sc.in_local_frame(pts, [100.0, 0.0, 0.0])
    np.testing.assert_array_equal(sc.voxel_keys(world, 1.0), sc.voxel_keys(pts, 1.0))
    o.Update(local, sc.translation([100.0, 0.0, 0.0]))
    pts = world
    assert o.num_voxels() == 200 and o.num_points() == 600
    q = sc.jittered_queries(pts, 1.0)
    nn, d = o.GetClosestNeighbor(q)
    assert (d < 0.5).sum() > 1000  # most queries have a neighbour near by
    np.testing.assert_array_equal(bucket_sorted(pts, 1.0), o.buckets())


def test_ordered_frames_claim_distinct_slots():
    """the premise of sc.ordered_frames: in both claim launches every new voxel takes a slot no other new voxel of the launch wants"""
    first, second = [sc.voxel_keys(f, 1.0) for f in sc.ordered_frames()]
    n1, n2 = len(first), len(second)
    assert (n1, n2) == (100, 300) and len(np.unique(np.concatenate([first, second]), axis=0)) == n1 + n2
    # the first frame: staged and too tight in the fresh table, so the table is re-hashed - empty - and claimed again
    assert sc.too_tight_premise(n1) == (True, True, True)
    want = 1024
    while (0 + 32 * n1 + 1024) * 4 > want:
        want *= 2
    assert want == sc.ORDERED_SLOTS
    filled = np.zeros(want, dtype=bool)
    s1 = sc.slots_taken_alone(filled, first)
    assert len(set(s1)) == n1
    filled[s1] = True
    # its apply step adds the 26 neighbours of every voxel (whatever their order: the SET of filled slots does not depend on it)
    shifts = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    halo = np.unique((first[:, None, :] + shifts[None]).reshape(-1, 3), axis=0)
    halo = halo[~(halo[:, None, :] == first[None]).all(-1).any(1)]
    for key in halo:
        filled[sc.slots_taken_alone(filled, key[None])] = True
    entries = int(filled.sum())
    # the second frame: no re-hash, room for the worst case - one queue, which a begin leaves pending
    assert (entries + n2) * 2 <= want and (entries + 27 * n2) * 4 <= 3 * want
    assert not (second[:, None, :] == np.concatenate([first, halo])[None]).all(-1).any()  # every voxel of it is a new entry
    assert len(set(sc.slots_taken_alone(filled, second))) == n2


def test_update_counts_of_a_map_that_never_left_the_host():
    """kicp_map_update_counts / kicp_map_device_updates read host-side counters only: they work without a GPU, and host-side calls
    leave all twelve at zero"""
    import kinematic_icp_amd as K
    m = K.VoxelHashMap(1.0, 30.0, 20)
    m.AddPoints(sc.isolated(30))
    m.Update(sc.isolated(30, centre=(9.0, 0.0, 0.0)), sc.IDENTITY)
    m.Clear()
    c = m.update_counts()
    assert list(c) == list(K.VoxelHashMap.UPDATE_COUNTS) and len(c) == 12 and not any(c.values())
    assert m.device_updates() == 0
