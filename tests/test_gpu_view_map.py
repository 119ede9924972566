"""The map sweep on the GPU (kicp_map_remove_seen_through: K.VoxelHashMap.RemoveSeenThrough) against the numpy restatement
(tests/view_ref.py: expected map = bucket_sorted(cloud)[~verdict]).  After EVERY sweep the map's buckets - points and their order -,
the four statistics, the counters and the table invariants must equal the restatement's, and GetClosestNeighbor must answer as an
oracle map rebuilt from the expected cloud does.  Everything is exact."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import mapdev_scenes as sc
import view_cases as vc
import view_ref as vr
from checkers import okicp
from mapdev_ref import bucket_sorted

pytestmark = pytest.mark.gpu

SWEEPS = vc.sweep_cases()
MAX_DISTANCE = 100.0


def make_view(cfg):
    return K.DepthView(cfg["res"], cfg["window"], cfg["min_rays"], cfg["max_ray"], cfg["margin"], cfg["margin_per_metre"])


@pytest.fixture(scope="module")
def wall():
    """the wall frame, its image and sensor position by the restatement - computed once, never changed"""
    frame = vc.wall()
    depth, stats, c = vr.render(vc.WALL_CFG, frame, vc.IDENTITY, vc.ORIGIN)
    depth.setflags(write=False)
    return dict(frame=frame, depth=depth, c=c, stats=stats)


def wall_view(wall):
    view = make_view(vc.WALL_CFG)
    assert view.render(wall["frame"], vc.IDENTITY, vc.ORIGIN) == wall["stats"]
    return view


def check_sweep(gmap, view, cfg, depth, c, before, vs, cap, rng, max_distance=MAX_DISTANCE):
    """sweep gmap, whose buckets are `before` (bucket-sorted): statistics, buckets, counters, invariants and neighbour lookups equal the
    restatement's -> (the expected cloud, an oracle map rebuilt from it, the statistics)"""
    keep, stats = vr.sweep(cfg, depth, c, before, vs)
    want = before[keep]
    got = gmap.RemoveSeenThrough(view)
    print("sweep: %d points, restatement %s, device %s" % (len(before), stats, got))
    assert got == stats
    assert gmap.num_points() == len(want)
    assert gmap.num_voxels() == (len(np.unique(np.floor(want / vs), axis=0)) if len(want) else 0)
    assert np.array_equal(bucket_sorted(gmap.Pointcloud(), vs), want)
    omap = okicp.VoxelHashMap(vs, max_distance, cap)
    omap.AddPoints(want)
    assert omap.num_points() == len(want)
    # lookups next to what left and what stayed: the removed points themselves, the survivors, and points around them
    gone = before[~keep]
    queries = np.concatenate([gone[:300], want[:300], want[:200] + rng.uniform(-0.7, 0.7, (min(200, len(want)), 3)), gone[:200] + rng.uniform(-1.2, 1.2, (min(200, len(gone)), 3)),
                              np.array([[500.0, 500.0, 500.0]])])
    nn, d = gmap.GetClosestNeighbor(queries)
    nn_o, d_o = omap.GetClosestNeighbor(queries)
    assert np.array_equal(nn, nn_o) and np.array_equal(d, d_o)
    assert gmap.check() == 0
    assert np.array_equal(bucket_sorted(gmap.Pointcloud(), vs), want)  # the host copy after the download
    return want, omap, stats


def build(case, device=True):
    gmap = K.VoxelHashMap(case["vs"], MAX_DISTANCE, case["cap"])
    if device:
        assert gmap.UpdateDevice(K.DeviceFrame(case["points"]), vc.IDENTITY)  # the HBM copy is the current one
    else:
        gmap.AddPoints(case["points"])
    assert gmap.num_points() == len(case["points"])
    return gmap, bucket_sorted(case["points"], case["vs"])


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_sweep_case(name, wall):
    """a bucket losing its first / a middle / its last point; a full bucket (20) losing everything - the voxel is erased, its neighbours'
    lookups stay right, a voxel out of range is untouched; max_points_per_voxel 150 (three trips per wave, alternating verdicts) and 300 (12
    count bits)"""
    case = SWEEPS[name]
    rng = np.random.default_rng(1)
    gmap, before = build(case)
    view = wall_view(wall)
    want, _, stats = check_sweep(gmap, view, vc.WALL_CFG, wall["depth"], wall["c"], before, case["vs"], case["cap"], rng)
    assert stats[1] == int(case["pattern"].sum()) > 0
    if name == "full_bucket_erased":
        assert stats == (len(case["points"]) - 1, 22, 2, 1) and np.any(np.all(want == [40.5, 0.5, 0.5], axis=1))
    # a second sweep with the same view finds nothing more to remove
    again, _, stats2 = check_sweep(gmap, view, vc.WALL_CFG, wall["depth"], wall["c"], want, case["vs"], case["cap"], rng)
    assert stats2[1:] == (0, 0, 0) and len(again) == len(want)
    # the freed and shortened buckets take points again as the oracle's do
    gmap.UpdateDevice(K.DeviceFrame(case["points"]), vc.IDENTITY)
    omap = okicp.VoxelHashMap(case["vs"], MAX_DISTANCE, case["cap"])
    omap.AddPoints(want)
    omap.Update(case["points"], vc.IDENTITY)
    assert np.array_equal(bucket_sorted(gmap.Pointcloud(), case["vs"]), bucket_sorted(omap.Pointcloud(), case["vs"])) and gmap.check() == 0


def test_empty_map_and_view_never_rendered(wall):
    gmap = K.VoxelHashMap(1.0, MAX_DISTANCE, 20)
    view = wall_view(wall)
    assert gmap.RemoveSeenThrough(view) == (0, 0, 0, 0) and gmap.num_points() == 0 and gmap.check() == 0
    case = SWEEPS["first_middle_last"]
    gmap, before = build(case)
    blank = make_view(vc.WALL_CFG)
    assert gmap.RemoveSeenThrough(blank) == (0, 0, 0, 0)
    assert np.array_equal(bucket_sorted(gmap.Pointcloud(), 1.0), before) and gmap.check() == 0
    gmap.Clear()
    assert gmap.RemoveSeenThrough(view) == (0, 0, 0, 0) and gmap.Empty()


def test_map_never_synced_to_the_device(wall):
    case = SWEEPS["full_bucket_erased"]
    gmap, before = build(case, device=False)  # host insertion: no mirror yet
    assert gmap.device_bytes() == 0
    check_sweep(gmap, wall_view(wall), vc.WALL_CFG, wall["depth"], wall["c"], before, case["vs"], case["cap"], np.random.default_rng(2))
    assert gmap.device_bytes() > 0 and gmap.update_counts()["host_updates"] == 0


def test_sweep_straight_after_update_begin(wall):
    """the pending update is collected first: its points are judged too"""
    case = SWEEPS["first_middle_last"]
    gmap, _ = build(dict(case, points=case["points"][:3]))
    frame = K.DeviceFrame(case["points"][3:])
    gmap.UpdateDeviceBegin(frame, vc.IDENTITY)
    before = bucket_sorted(case["points"], case["vs"])
    _, _, stats = check_sweep(gmap, wall_view(wall), vc.WALL_CFG, wall["depth"], wall["c"], before, case["vs"], case["cap"], np.random.default_rng(3))
    assert stats[1] == 3 and gmap.update_counts()["deferred"] == 1 and gmap.UpdateFinish()


def test_host_only_map_gives_the_same_result(wall):
    """a point beyond +-2^20 voxels keeps the map's updates on the host: the sweep runs there, with the same verdict"""
    case = SWEEPS["full_bucket_erased"]
    points = np.concatenate([case["points"], [[2.0e6, 0.0, 0.0]]])
    gmap = K.VoxelHashMap(case["vs"], MAX_DISTANCE, case["cap"])
    gmap.AddPoints(points)
    view = wall_view(wall)
    want, _, stats = check_sweep(gmap, view, vc.WALL_CFG, wall["depth"], wall["c"], bucket_sorted(points, case["vs"]), case["vs"], case["cap"], np.random.default_rng(4))
    assert stats == (len(case["points"]) - 1, 22, 2, 1)
    on_device, before = build(case)
    assert on_device.RemoveSeenThrough(view) == stats
    assert np.array_equal(bucket_sorted(on_device.Pointcloud(), 1.0), want[:-1])  # (the far point sorts last)
    assert not gmap.UpdateDevice(K.DeviceFrame(case["points"][:5]), vc.IDENTITY)  # still a host map afterwards
    assert gmap.check() == 0


def test_registration_on_the_swept_map_equals_a_fresh_map():
    """ComputeRobotMotion on the swept map returns the bit-equal pose of a fresh map built from the expected cloud"""
    d = vc.reference_drive()
    fr, step = d["frames"][4], d["steps"]
    gmap = K.VoxelHashMap(vc.DRIVE_VS, vc.DRIVE_MAX_RANGE, vc.DRIVE_CAP)
    gmap.AddPoints(step[3]["after_update"])
    assert gmap.num_points() == len(step[3]["after_update"])
    view = make_view(vc.DRIVE_CFG)
    assert view.render(fr["frame"], fr["pose"], fr["sensor"]) == step[4]["render_stats"]
    assert gmap.RemoveSeenThrough(view) == step[4]["sweep_stats"] and step[4]["sweep_stats"][1] > 0
    fresh = K.VoxelHashMap(vc.DRIVE_VS, vc.DRIVE_MAX_RANGE, vc.DRIVE_CAP)
    fresh.AddPoints(step[4]["after_sweep"])
    assert np.array_equal(bucket_sorted(gmap.Pointcloud(), vc.DRIVE_VS), step[4]["after_sweep"])
    from kinematic_icp_amd import synthetic as syn
    rel = syn.planar_pose(0.45, 0.0, np.deg2rad(1.5))
    last = syn.pose_mul(fr["pose"], syn.pose_inverse(rel))
    reg = K.KinematicRegistration(device=0)
    a = reg.ComputeRobotMotion(fr["frame"][::4], gmap, last, rel, 0.5)
    b = reg.ComputeRobotMotion(fr["frame"][::4], fresh, last, rel, 0.5)
    assert reg.last_stats.iterations >= 1 and np.array_equal(a, b)


def test_pinned_drive_frame_by_frame():
    """The 8-frame drive with a person walking through, at the true poses: render_device + RemoveSeenThrough + UpdateDevice must equal the
    restatement frame by frame, so the conditions tests/test_view_host.py holds the restatement to carry over.  Freed buckets are reused
    from frame to frame, the order inside every bucket is kept."""
    d = vc.reference_drive()
    gmap = K.VoxelHashMap(vc.DRIVE_VS, vc.DRIVE_MAX_RANGE, vc.DRIVE_CAP)
    view = make_view(vc.DRIVE_CFG)
    for k, (fr, step) in enumerate(zip(d["frames"], d["steps"])):
        frame = K.DeviceFrame(fr["frame"])
        assert view.render_device(frame, fr["pose"], fr["sensor"]) == step["render_stats"]
        assert gmap.RemoveSeenThrough(view) == step["sweep_stats"], k
        if k in (3, 7):
            assert np.array_equal(view.depth(), step["depth"])
            assert np.array_equal(bucket_sorted(gmap.Pointcloud(), vc.DRIVE_VS), step["after_sweep"]), k
        assert gmap.UpdateDevice(frame, fr["pose"])
        assert gmap.num_points() == len(step["after_update"]), k
    assert np.array_equal(bucket_sorted(gmap.Pointcloud(), vc.DRIVE_VS), d["final"])
    assert gmap.check() == 0 and gmap.update_counts()["host_updates"] == 0
    assert sum(s["sweep_stats"][3] for s in d["steps"]) > 0  # voxels were erased along the way


def test_update_sweep_update_sweep_and_a_rehash(wall):
    """update -> sweep -> update -> sweep over several frames, the oracle map rebuilt after each sweep (freed buckets reused, order kept),
    then enough insertions to force a device re-hash, and one more sweep"""
    rng = np.random.default_rng(6)
    vs, cap = 1.0, 20
    gmap = K.VoxelHashMap(vs, MAX_DISTANCE, cap)
    view = wall_view(wall)
    omap = okicp.VoxelHashMap(vs, MAX_DISTANCE, cap)
    removed = 0
    for k in range(4):
        # points on both sides of the line x = 10.098 in front of the wall, and some outside its cone
        pts = np.stack([rng.uniform(9.6, 10.6, 400), rng.uniform(-4.0, 4.0, 400), rng.uniform(-2.5, 2.5, 400)], axis=1)
        assert gmap.UpdateDevice(K.DeviceFrame(pts), vc.IDENTITY)
        omap.Update(pts, vc.IDENTITY)
        before = bucket_sorted(omap.Pointcloud(), vs)
        assert np.array_equal(bucket_sorted(gmap.Pointcloud(), vs), before)
        want, omap, stats = check_sweep(gmap, view, vc.WALL_CFG, wall["depth"], wall["c"], before, vs, cap, rng)
        removed += stats[1]
        assert stats[1] > 0 and stats[3] > 0
    rehashes = gmap.update_counts()["rehashes"]
    for k in range(40):  # spread-out voxels until the table has to grow
        pts = rng.uniform(-60, 60, (3000, 3))
        assert gmap.UpdateDevice(K.DeviceFrame(pts), vc.IDENTITY)
        omap.Update(pts, vc.IDENTITY)
        if gmap.update_counts()["rehashes"] > rehashes:
            break
    assert gmap.update_counts()["rehashes"] > rehashes
    before = bucket_sorted(omap.Pointcloud(), vs)
    assert np.array_equal(bucket_sorted(gmap.Pointcloud(), vs), before)
    check_sweep(gmap, view, vc.WALL_CFG, wall["depth"], wall["c"], before, vs, cap, rng)


def test_sweep_straight_after_an_update_that_rehashed_and_grew_the_pools(wall):
    """the first device update into a fresh map (tests/test_gpu_mapdev_regimes.py's n = 8 192, region 0 scene) replaces the table, the key
    array and both pools; the sweep that follows must see the new ones"""
    vs, cap, max_distance = 1.0, 20, 150.0
    s = sc.one_per_voxel(8192, 0, 1000)
    t = sc.region_centre(0)
    local, _ = sc.in_local_frame(s["points"], t)
    gmap = K.VoxelHashMap(vs, max_distance, cap)
    c0 = gmap.update_counts()
    assert gmap.UpdateDevice(K.DeviceFrame(local), sc.translation(t))
    c1 = gmap.update_counts()
    assert (c1["rehashes"] - c0["rehashes"], c1["pool_growths"] - c0["pool_growths"], c1["one_queue"], c1["host_updates"]) == (1, 1, 1, 0)
    omap = okicp.VoxelHashMap(vs, max_distance, cap)
    omap.Update(local, sc.translation(t))
    before = bucket_sorted(omap.Pointcloud(), vs)
    assert len(before) == 8192 + 1000 == gmap.num_points()
    _, _, stats = check_sweep(gmap, wall_view(wall), vc.WALL_CFG, wall["depth"], wall["c"], before, vs, cap, np.random.default_rng(7), max_distance)
    assert stats[1] > 0 and stats[3] > 0 and gmap.update_counts()["host_updates"] == 0  # points left, voxels were erased, all on the device
