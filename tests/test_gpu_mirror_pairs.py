"""Every way a mirror row reaches the device and comes back, on the scenes of tests/mirror_z_cases.py (buckets of 1, 19, 20, 21 and 40
points, z equal to 0 and 65 535, buckets emptied and re-used; premises() proves each regime on the CPU).  Written for a device layout
that pairs the words of two points per 16 bytes (x|y, x|y, z, z), which every one of these paths had to convert or address; that layout
lost its A/B and is not in the tree (profiles/visit_trim_ab.txt), the test holds whatever layout the device keeps to the same
outcome - and passed with the paired one.  Every scene is built three ways:

    whole     on the host, uploaded whole (the full upload)
    staged    on the host without the last point of three buckets, synced, those three buckets extended, synced again: the partial-row
              upload (asserted: the second upload is a delta; the scenes of five buckets extend two and the one of two buckets one -
              a third would change more than half of the buckets, and the map then re-sends everything)
    device    by UpdateDevice (the append sites and row resets of the map update)

After each build the map is downloaded and the host check() holds every mirror word of the host's rows to its fp64 point: 0 bad, and
the buckets are the model's point for point.  For every build of the pass kernel a handle can pick the
correspondences equal the oracle's index for index and the sums are bit-equal across kernel builds and across the three ways; a batch
through the job list returns the bits of the single calls.  A k_view_sweep removal that leaves 23 of 31 points in a two-trip bucket
(odd count, removals at slot 0, at odd and even slots and at the end) goes through the same checks.  The helpers and the kernel builds are
those of tests/test_gpu_mirror_z.py; the oracle's results are computed once per scene."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import mirror_z_cases as mc
import test_gpu_mirror_z as tz
import view_cases as vc
import view_ref as vr
from checkers import okicp
from mapdev_ref import bucket_sorted

pytestmark = pytest.mark.gpu
I, TAU = mc.IDENTITY, mc.TAU
ROUTES = ["whole", "staged", "device"]


@pytest.fixture(scope="module")
def world():
    return tz.World()


def _held_back(points):
    """indices of the last point of three voxels that hold at least two points of `points` (their buckets get extended, not created)"""
    vox = np.floor(points / mc.VS).astype(np.int64)
    last, count = {}, {}
    for i, v in enumerate(map(tuple, vox)):
        last[v], count[v] = i, count.get(v, 0) + 1
    # (three where the scene has seven buckets or more; fewer in the smaller scenes, where a third changed bucket would turn the delta
    #  into a full upload - more than half of the buckets changed - or where fewer voxels hold two points)
    picks = sorted(last[v] for v in last if count[v] >= 2)[:min(3, len(last) // 2)]
    assert len(picks) >= 1
    return picks


def walk(world, name, route):
    """tests/test_gpu_mirror_z.py's walk with a third route; yields (state, map) after holding invariants and buckets to the model"""
    if route == "device":
        yield from tz.walk(world, name, "device")
        return
    scene = world.scenes[name]
    gmap = K.VoxelHashMap(mc.VS, scene.max_distance, scene.cap)
    for k, step in enumerate(scene.steps):
        if step[0] == "update":
            _, points, origin = step
            if route == "staged" and k == 0:
                held = _held_back(points)
                gmap.AddPoints(np.delete(points, held, axis=0))
                gmap.sync(0)
                gmap.AddPoints(points[held])   # three buckets grow by their last point
                gmap.RemovePointsFarFromLocation(origin)
                gmap.sync(0)
                assert not gmap.last_upload()[1]  # a delta: the staged rows
            else:
                gmap.AddPoints(points)
                gmap.RemovePointsFarFromLocation(origin)
                if k == 0:
                    gmap.sync(0)
                    assert gmap.last_upload()[1]  # the whole map
        else:
            cfg = vc.WALL_CFG
            view = K.DepthView(cfg["res"], cfg["window"], cfg["min_rays"], cfg["max_ray"], cfg["margin"], cfg["margin_per_metre"])
            assert view.render(world.wall[0], vc.IDENTITY, vc.ORIGIN) == world.wall[3]
            assert gmap.RemoveSeenThrough(view)[3] >= 1
        if k + 1 in scene.looks:
            state = scene.looks[k + 1]
            model = world.states[name][state][0]
            assert gmap.check() == 0
            assert np.array_equal(bucket_sorted(gmap.Pointcloud(), mc.VS), bucket_sorted(model.points(), mc.VS))
            yield state, gmap
            assert gmap.check() == 0


@pytest.mark.parametrize("name", tz.SCENES)
def test_three_ways_to_build_a_map_give_every_kernel_the_oracles_points(world, name):
    scene = world.scenes[name]
    seen = {}
    for route in ROUTES:
        looks = 0
        for state, gmap in walk(world, name, route):
            q = scene.queries[state]
            for build, options in tz.BUILDS:
                idx, sums = tz._check_build(options, gmap, scene.cap, q, world.want(name, state))
                first = seen.setdefault(state, (idx % scene.cap, sums))  # (bucket numbers may differ between the ways; the slot may not)
                assert np.array_equal(np.where(idx >= 0, idx % scene.cap, -1), np.where(idx >= 0, first[0], -1)), (route, build)
                assert np.array_equal(sums, first[1]), (route, build)
            # downloaded: the host's rows hold every point's words (check() compares each with mirror_point of its fp64 point)
            twin = gmap.copy()
            assert twin.check() == 0 and np.array_equal(bucket_sorted(twin.Pointcloud(), mc.VS), bucket_sorted(gmap.Pointcloud(), mc.VS))
            looks += 1
        assert looks == len(scene.looks)


@pytest.mark.parametrize("route", ROUTES)
def test_a_batch_of_two_scans_through_the_job_list(world, route):
    """two distinct scans (the whole scan and every other query) nine times over: groups of four jobs on two lanes"""
    name = "trips40"
    scene = world.scenes[name]
    for state, gmap in walk(world, name, route):
        q = scene.queries[state]
        scans = [q, np.ascontiguousarray(q[::2])] * 9
        reg = tz._reg(tz.GROUPED)
        b = reg.prepare_batch([K.DeviceFrame(s, device=0) for s in scans], [I] * len(scans), [I] * len(scans))
        got = reg.ComputeRobotMotionBatch(b, gmap, TAU).copy()
        assert reg.get_option("batch_group_launches") > 0
        single = tz._reg(tz.FOUR_WAVES)
        for k in range(2):
            pose = single.ComputeRobotMotion(scans[k], gmap, I, I, TAU)
            for j in range(k, len(scans), 2):
                assert np.array_equal(got[j], pose, equal_nan=True) and int(b.iterations[j]) == single.last_stats.iterations


@pytest.mark.parametrize("route", ["whole", "device"])
def test_a_sweep_leaves_an_odd_count_in_a_two_trip_bucket(route):
    """31 points in voxel (10, 0, 0) of a map with 40 points per voxel; the wall's frame sees through eight of them - slots 0, 3, 4, 11,
    20, 21, 29 and 30: the sweep compacts 23 points over pairs it has half vacated, and empties slots 23 .. 30"""
    gone = {0, 3, 4, 11, 20, 21, 29, 30}
    pattern = [i in gone for i in range(31)]
    pts = np.concatenate([vc.bucket(pattern, 0, 0, 40), vc.bucket([False] * 5, 1, 0, 40)])
    kept = np.concatenate([pts[:31][~np.array(pattern)], pts[31:]])
    gmap = K.VoxelHashMap(1.0, 100.0, 40)
    if route == "whole":
        gmap.AddPoints(pts)
    else:
        assert gmap.UpdateDevice(K.DeviceFrame(pts), vc.IDENTITY)
    assert gmap.num_points() == 36
    frame = vc.wall()
    _, stats, _ = vr.render(vc.WALL_CFG, frame, vc.IDENTITY, vc.ORIGIN)
    cfg = vc.WALL_CFG
    view = K.DepthView(cfg["res"], cfg["window"], cfg["min_rays"], cfg["max_ray"], cfg["margin"], cfg["margin_per_metre"])
    assert view.render(frame, vc.IDENTITY, vc.ORIGIN) == stats
    removed = gmap.RemoveSeenThrough(view)
    assert removed[1] == 8 and removed[2] == 1 and removed[3] == 0
    assert gmap.num_points() == 28 and gmap.check() == 0
    cloud = gmap.Pointcloud()
    assert np.array_equal(bucket_sorted(cloud, 1.0), bucket_sorted(kept, 1.0))
    omap = okicp.VoxelHashMap(1.0, 100.0, 40)
    omap.AddPoints(kept)
    rng = np.random.default_rng(2)
    q = np.concatenate([kept + rng.uniform(-0.02, 0.02, kept.shape), pts[:31][np.array(pattern)] + 0.01])  # at every kept point, and where the removed ones were
    acc, onn, od = okicp.associate(omap, q, I, TAU)
    assert acc[:len(kept)].all()
    osums, _ = okicp.icp_pass(omap, q, I, TAU)
    first = None
    for build, options in tz.BUILDS:
        reg = tz._reg(options)
        idx, d2, nn = reg.pass_correspondences(q, gmap, I, TAU)
        np.testing.assert_array_equal(idx >= 0, acc, err_msg=build)
        np.testing.assert_array_equal(nn[acc], onn[acc], err_msg=build)
        np.testing.assert_array_equal(np.sqrt(d2[acc]), od[acc], err_msg=build)
        sums = reg.pass_sums(q, gmap, I, TAU)
        np.testing.assert_allclose(sums, osums, rtol=tz.SUM_RTOL, atol=1e-9)
        first = first if first is not None else sums
        assert np.array_equal(sums, first), build
    # the bucket takes points again behind the sweep: the emptied slots are empty
    more = np.array([[10.9, 0.5, 0.5]])
    assert gmap.UpdateDevice(K.DeviceFrame(more), vc.IDENTITY)
    omap.AddPoints(more)
    assert gmap.num_points() == omap.num_points() == 29 and gmap.check() == 0
    idx, d2, nn = tz._reg(tz.FOUR_WAVES).pass_correspondences(q, gmap, I, TAU)
    acc, onn, od = okicp.associate(omap, q, I, TAU)
    np.testing.assert_array_equal(idx >= 0, acc)
    np.testing.assert_array_equal(nn[acc], onn[acc])
