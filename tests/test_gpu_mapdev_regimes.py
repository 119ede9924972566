"""VoxelHashMap::Update on the GPU (kicp_mapdev.hpp, map_update_device in kicp_map_update.hip) in the regimes the drive-through tests of
tests/test_gpu_mapdev.py never enter: more than 8 192 touched voxels in the one-workgroup scan, the size edges of the one-queue
path, buckets deeper than a wave, the acceptance and pruning radii met exactly, the "too tight" second claim, the free list emptied,
refilled and handed between host and device.  Every test drives K.VoxelHashMap and the oracle(s) in lock step (mapdev_ref.Oracles);
after EVERY update: equal counts, the same points in the same order in every bucket (on the device-gathered cloud and on the
downloaded host copy) and check() == 0; at the end GetClosestNeighbor bit for bit on ~2 000 jittered queries and one pass_sums on
the device copy (accepted count exactly, sums to the 1e-10 of test_pass_sums_match_oracle) - the masks and the 16-bit mirror the
pass kernels read.  Each test asserts from update_counts() that it took the path it is named after, so that a moved threshold fails
here instead of silently uncovering the path.  The scenes' premises are proved on the CPU in tests/test_mapdev_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import mapdev_scenes as sc
from checkers import okicp
from mapdev_ref import Oracles, assert_same_buckets, bucket_sorted

pytestmark = pytest.mark.gpu
SUM_RTOL = 1e-10  # tests/test_gpu_parity.py test_pass_sums_match_oracle


@pytest.fixture(scope="module")
def reg():
    return K.KinematicRegistration()


def rose(before, after, **deltas):
    """the named counters moved by exactly the given amounts"""
    for name, d in deltas.items():
        assert after[name] - before[name] == d, "%s moved by %d, not %d (%s -> %s)" % (name, after[name] - before[name], d, before, after)


class Lockstep:
    """One device-maintained map and the oracle(s), updated together and compared after every update"""

    def __init__(self, vs, max_distance, cap, device=None):
        self.vs = vs
        self.g = K.VoxelHashMap(vs, max_distance, cap, device=device)
        self.o = Oracles(vs, max_distance, cap)
        self.frames = []  # (a deferred update borrows its frame)
        self.updates = 0

    def counts(self):
        return self.g.update_counts()

    def compare(self):
        self.updates += 1
        msg = "update %d" % self.updates
        assert (self.g.num_points(), self.g.num_voxels()) == (self.o.num_points(), self.o.num_voxels()), msg
        assert_same_buckets(self.g, self.o, self.vs, msg)

    def update_device(self, local, pose, how="device"):
        """UpdateDevice (how = "device") or UpdateDeviceBegin + UpdateFinish ("deferred"); -> (counters before, after the begin, at the end)"""
        frame = K.DeviceFrame(local)
        self.frames.append(frame)
        c0 = self.counts()
        if how == "device":
            assert self.g.UpdateDevice(frame, pose)
            c1 = self.counts()
        else:
            self.g.UpdateDeviceBegin(frame, pose)
            c1 = self.counts()
            assert self.g.UpdateFinish()
        self.o.Update(local, pose)
        c2 = self.counts()
        rose(c0, c2, host_updates=0)
        self.compare()
        return c0, c1, c2

    def add_points(self, world):
        self.g.AddPoints(world), self.o.AddPoints(world)
        self.compare()

    def remove_far_on_host(self, origin):
        self.g.RemovePointsFarFromLocation(origin), self.o.RemovePointsFarFromLocation(origin)
        self.compare()

    def finale(self, reg, tau=None):
        cloud = self.o.o.Pointcloud()
        q = sc.jittered_queries(cloud, self.vs)
        nn_g, d_g = self.g.GetClosestNeighbor(q)
        nn_o, d_o = self.o.GetClosestNeighbor(q)
        assert np.array_equal(d_g, d_o) and np.array_equal(nn_g, nn_o)
        tau = 0.5 * self.vs if tau is None else tau
        got = reg.pass_sums(q, self.g, sc.IDENTITY, tau)
        want, _ = okicp.icp_pass(self.o.o, q, sc.IDENTITY, tau)
        assert got[6] == want[6] and (len(cloud) == 0 or want[6] > 0), (got, want)
        np.testing.assert_allclose(got, want, rtol=SUM_RTOL, atol=1e-9)


# ---- scan chunks and size edges ---------------------------------------------------------------------------------------
# (n voxels, extras): the scene has n + 2 * extras points.  k_up_scan's chunk is 8 192 TOUCHED VOXELS, the one-queue path takes up to
# 16 384 POINTS: 8 192 / 8 193 voxels sit on the first edge with rejected and accepted extras on top, 14 384 + 2 000 and 16 384 + 0
# points sit on the second from below (the latter with as many voxels as points).
@pytest.mark.parametrize("n,extras", [(8192, 1000), (8193, 1000), (12288, 1000), (14384, 1000), (16384, 0)])
def test_scan_chunks_and_size_edges_one_queue(reg, n, extras):
    L = Lockstep(1.0, 150.0, 20)  # (150: a region's own corners are 91 from its centre, the next region 236)
    for region, how in ((0, "device"), (1, "device"), (2, "deferred")):
        s = sc.one_per_voxel(n, region, extras)
        t = sc.region_centre(region)
        local, _ = sc.in_local_frame(s["points"], t)
        c0, c1, c2 = L.update_device(local, sc.translation(t), how)
        assert len(local) <= 16384 and c2["touched"] == n  # (more than one scan chunk for n > 8 192)
        # the update at this region's centre pruned the region before: region 2's voxels pop region 0's buckets from the free list
        assert L.g.num_voxels() == n and L.g.num_points() == n + extras
        if region == 0:  # a fresh map: the table is re-hashed to size and the pools are allocated first
            rose(c0, c2, rehashes=1, pool_growths=1, one_queue=1, staged=0, apply_wave=1, apply_thread=0, wide_scans=0, deferred=0)
        else:
            rose(c0, c2, one_queue=1, staged=0, second_claims=0, rehashes=0, apply_wave=1, apply_thread=0, wide_scans=0,
                 deferred=int(how == "deferred"))
            rose(c0, c1, deferred=int(how == "deferred"))
    L.finale(reg)


def test_size_edge_16385_points_takes_the_staged_path(reg):
    n = 16385
    L = Lockstep(1.0, 150.0, 20)
    for region, how in ((0, "device"), (1, "device"), (2, "deferred")):
        s = sc.one_per_voxel(n, region, 0)
        t = sc.region_centre(region)
        local, _ = sc.in_local_frame(s["points"], t)
        c0, c1, c2 = L.update_device(local, sc.translation(t), how)
        # too many points for one queue (a begin runs to completion), too many touched voxels for the wave-per-voxel kernel
        rose(c0, c2, staged=1, one_queue=0, wide_scans=1, apply_thread=1, apply_wave=0, deferred=0, second_claims=0)
        assert c2["touched"] == n and L.g.num_voxels() == n
    L.finale(reg)


# ---- deep buckets in the wave kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [64, 65, 128, 255])
def test_deep_buckets_in_the_wave_kernel(reg, cap):
    s = sc.deep_voxels(cap)
    pts = s["points"]
    L = Lockstep(1.0, 30.0, cap)
    # 24 000 offers, ~600 per voxel: groups far longer than a wave, buckets filling past 64 inside one launch
    c0, _, c2 = L.update_device(pts[:24000], sc.IDENTITY)
    rose(c0, c2, staged=1, wide_scans=1, apply_wave=1, apply_thread=0)
    assert c2["touched"] == 40 and L.g.num_voxels() == 40
    # 6 000 more into the same voxels: the old buckets (up to `cap` points) are preloaded into LDS
    c0, _, c2 = L.update_device(pts[24000:], sc.IDENTITY)
    rose(c0, c2, one_queue=1, apply_wave=1, apply_thread=0, staged=0)
    assert c2["touched"] == 40 and L.g.num_points() >= 40 * min(cap, 250)
    # 100 m away with range 30: everything is pruned, and 200 voxels of 3 points re-use the 40 freed deep buckets (and 160 fresh ones);
    # check() proves that the re-used buckets' mirror reads empty behind their three points
    t = np.array([100.0, 0.0, 0.0])
    local, _ = sc.in_local_frame(sc.shallow_voxels(40, t), t)
    c0, _, c2 = L.update_device(local, sc.translation(t))  # (the pruning runs behind the insertion: these 40 take fresh buckets)
    assert L.g.num_voxels() == 40 and L.g.num_points() == 120
    local, _ = sc.in_local_frame(sc.shallow_voxels(200, t + [0.0, 12.0, 0.0]), t)
    c0, _, c2 = L.update_device(local, sc.translation(t))
    rose(c0, c2, one_queue=1, apply_wave=1, apply_thread=0, pool_growths=0)
    assert c2["touched"] == 200 and L.g.num_voxels() == 240 and L.g.num_points() == 720
    L.finale(reg)


# ---- radius ties and faces --------------------------------------------------------------------------------------------------
LATTICES = [("radius", vs, cap) for vs, cap in sc.RADIUS_LATTICES] + [("division", 0.1, 20), ("division", 0.3, 20)]


@pytest.mark.parametrize("kind,vs,cap", LATTICES)
def test_radius_ties_and_voxel_faces(reg, kind, vs, cap):
    s = sc.radius_lattice(vs, cap) if kind == "radius" else sc.division_lattice(vs, cap)
    pts, step = s["points"], s["res"] if kind == "radius" else vs
    for t in (np.zeros(3), np.array([3.0, -5.0, 1.0]) * step):
        pose = sc.translation(t)
        clouds = []
        for way in ("device", "bulk", "thirds"):
            L = Lockstep(vs, 1e6, cap, device=0 if way == "bulk" else None)
            c0 = L.counts()
            if way == "device":
                L.update_device(pts, pose)
            elif way == "bulk":  # AddPoints of a host array goes through HBM from 4 096 points on: every scene here has them
                L.add_points(pts + t)
                assert len(pts) >= 4096 and K.lib().kicp_map_last_update_on_device(L.g._h) == 1
            else:
                for part in np.array_split(pts, 3):
                    L.update_device(part, pose)
            c2 = L.counts()
            rose(c0, c2, host_updates=0, apply_thread=0)
            assert c2["apply_wave"] - c0["apply_wave"] == {"device": 1, "bulk": 1, "thirds": 3}[way]
            clouds.append(bucket_sorted(L.g.Pointcloud(), vs))
            L.finale(reg, tau=1.5 * step)
        np.testing.assert_array_equal(clouds[0], clouds[1]), np.testing.assert_array_equal(clouds[0], clouds[2])


# ---- the pruning radius met exactly ---------------------------------------------------------------------------------------------
def test_prune_edge_on_the_device_and_on_the_host(reg):
    s = sc.prune_edge()
    pts, keep = s["points"], s["keep"]
    A = Lockstep(1.0, s["max_distance"], s["cap"])
    c0, _, c2 = A.update_device(pts, sc.IDENTITY)  # k_up_remove decides
    rose(c0, c2, apply_wave=1)
    B = Lockstep(1.0, s["max_distance"], s["cap"], device=0)
    B.add_points(pts)  # a bulk insertion on the device, no pruning ...
    assert K.lib().kicp_map_last_update_on_device(B.g._h) == 1 and B.g.num_points() == len(pts)
    B.remove_far_on_host(np.zeros(3))  # ... then the host map's RemovePointsFarFromLocation on the downloaded copy
    a, b = bucket_sorted(A.g.Pointcloud(), 1.0), bucket_sorted(B.g.Pointcloud(), 1.0)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, bucket_sorted(pts[keep], 1.0))  # exactly-25 voxels gone, one ulp inside kept, first point decides
    A.finale(reg), B.finale(reg)


# ---- too tight: claim, re-hash, claim again -------------------------------------------------------------------------------------
def test_too_tight_retry(reg):
    assert sc.too_tight_premise(30) == (True, True, True)
    L = Lockstep(1.0, 1e6, 20)
    c0, _, c2 = L.update_device(sc.isolated(30), sc.IDENTITY)
    rose(c0, c2, staged=1, second_claims=1, rehashes=1, one_queue=0, apply_wave=1)
    assert c2["touched"] == 30 and L.g.num_voxels() == 30
    c0, _, c2 = L.update_device(sc.isolated(30, centre=(50.0, 0.0, 0.0), seed=1), sc.IDENTITY)  # the re-hashed table has the room
    rose(c0, c2, second_claims=0, rehashes=0, staged=0, one_queue=1, apply_wave=1)
    assert L.g.num_voxels() == 60
    L.finale(reg)


# ---- the free list, three ways ----------------------------------------------------------------------------------------------------
def _patch(L, n_voxels, pose_t, offset, how="device"):
    """n_voxels new voxels of 3 points beside pose_t + offset, inserted by an update at pose_t (which prunes what is 30 m from there)"""
    t = np.asarray(pose_t, dtype=np.float64)
    local, _ = sc.in_local_frame(sc.shallow_voxels(n_voxels, t + offset, seed=L.updates), t)
    return L.update_device(local, sc.translation(t), how)


def test_free_list_shorter_than_the_update_needs(reg):
    L = Lockstep(1.0, 30.0, 20)
    a, b = np.zeros(3), np.array([100.0, 0.0, 0.0])
    _patch(L, 100, a, [0.0, 0.0, 0.0])
    _patch(L, 10, b, [0.0, -14.0, 0.0])  # prunes the 100 on the device: 100 buckets on the free list
    assert L.g.num_voxels() == 10
    c0, _, c2 = _patch(L, 300, b, [0.0, 8.0, 0.0])  # 100 re-used buckets and 200 fresh ones in one launch
    rose(c0, c2, one_queue=1, apply_wave=1)
    assert L.g.num_voxels() == 310 and c2["touched"] == 300
    _patch(L, 300, a, [0.0, 0.0, 0.0], "deferred")  # everything pruned ...
    _patch(L, 350, a, [0.0, 0.0, 2.0])  # ... and refilled: 310 from the list, 40 fresh
    assert L.g.num_voxels() == 650
    L.finale(reg)


def test_free_list_filled_by_host_pruning_is_popped_on_the_device(reg):
    L = Lockstep(1.0, 30.0, 20)
    a, b = np.zeros(3), np.array([100.0, 0.0, 0.0])
    _patch(L, 150, a, [0.0, 0.0, 0.0])
    L.remove_far_on_host(b)  # the host map frees all 150 buckets
    assert L.g.num_voxels() == 0
    c0, _, c2 = _patch(L, 100, b, [0.0, 0.0, 0.0])  # the uploaded free list is popped by the device update
    rose(c0, c2, host_updates=0, apply_wave=1)
    assert L.g.num_voxels() == 100
    L.finale(reg)


def test_free_list_alternating_device_and_host_pruning(reg):
    L = Lockstep(1.0, 30.0, 20)
    _patch(L, 200, np.zeros(3), [0.0, 0.0, 0.0])
    before = L.counts()
    for k in range(1, 7):
        t = np.array([100.0 * k, 0.0, 0.0])
        if k % 2:  # device: a small update at the new place prunes the old one, then one that needs more buckets than were freed
            _patch(L, 10, t, [0.0, -14.0, 0.0], "deferred" if k == 3 else "device")
            _patch(L, 300, t, [0.0, 8.0, 0.0])
            assert L.g.num_voxels() == 310
        else:  # host: RemovePointsFarFromLocation frees everything, the device update pops fewer buckets than the list holds
            L.remove_far_on_host(t)
            assert L.g.num_voxels() == 0
            _patch(L, 120, t, [0.0, 0.0, 0.0])
            assert L.g.num_voxels() == 120
    rose(before, L.counts(), host_updates=0, staged=0, second_claims=0, apply_thread=0, deferred=1, one_queue=9)
    L.finale(reg)


# ---- kicp_map_device_updates does not collect -----------------------------------------------------------------------------------
def test_device_updates_does_not_collect_a_pending_update():
    L = Lockstep(1.0, 30.0, 20)
    _patch(L, 100, np.zeros(3), [0.0, 0.0, 0.0])
    before, c0 = L.g.device_updates(), L.counts()
    assert before == 1
    local = sc.shallow_voxels(50, [0.0, 8.0, 0.0], seed=5)
    frame = K.DeviceFrame(local)
    L.g.UpdateDeviceBegin(frame, sc.IDENTITY)
    rose(c0, L.counts(), deferred=1, one_queue=1)  # the update really is pending
    assert L.g.device_updates() == before  # include/kicp.h: the one call that does not wait for it
    assert L.g.update_counts()["deferred"] == c0["deferred"] + 1 and L.g.device_updates() == before  # nor does update_counts()
    assert L.g.UpdateFinish()
    assert L.g.device_updates() == before + 1
    L.o.Update(local, sc.IDENTITY)
    assert L.counts()["touched"] == 50
    L.compare()
    # Clear() empties the map and keeps the counters
    c = L.counts()
    assert c["deferred"] == 1 and c["apply_wave"] == 2 and c["rehashes"] >= 1
    L.g.Clear()
    assert L.g.Empty() and L.counts() == c and L.g.device_updates() == before + 1


# ---- the fp64 Pointcloud() collects a pending update ---------------------------------------------------------------------------------
def test_pointcloud_between_begin_and_finish_equals_the_twins_cloud():
    """Pointcloud() between UpdateDeviceBegin and UpdateFinish: the cloud of a twin map that took the same two frames through UpdateDevice,
    bit for bit and in the same order (sc.ordered_frames: frames whose table order is settled), and by the counters the pending update
    was collected and counted and the host map took nothing over.  This pins the answer, not the road to it: the fall-back through the
    host copy, which answered before kicp_map_pointcloud collected a pending update itself, leaves the same cloud and counters."""
    first, second = sc.ordered_frames()
    maps = [K.VoxelHashMap(1.0, 1000.0, 20) for _ in range(2)]
    for g in maps:
        c0 = g.update_counts()
        assert g.UpdateDevice(K.DeviceFrame(first), sc.IDENTITY)
        rose(c0, g.update_counts(), staged=1, second_claims=1, rehashes=1, host_updates=0)  # (the table sc.ORDERED_SLOTS stands for)
    pending, twin = maps
    frame = K.DeviceFrame(second)
    c0, before = pending.update_counts(), pending.device_updates()
    pending.UpdateDeviceBegin(frame, sc.IDENTITY)
    rose(c0, pending.update_counts(), deferred=1, one_queue=1)
    assert pending.device_updates() == before == 1  # the update really is pending
    # (K.VoxelHashMap.Pointcloud asks for num_points() first, which collects: kicp_map_pointcloud itself is called here)
    cloud = np.empty((400, 3))
    assert K.lib().kicp_map_pointcloud(pending._h, cloud.ctypes.data_as(C.POINTER(C.c_double)), 400) == 400
    rose(c0, pending.update_counts(), deferred=1, host_updates=0)
    assert pending.device_updates() == before + 1
    assert twin.UpdateDevice(K.DeviceFrame(second), sc.IDENTITY)
    want = twin.Pointcloud()
    assert cloud.shape == want.shape == (400, 3) and np.array_equal(cloud, want)
    assert np.array_equal(bucket_sorted(cloud, 1.0), bucket_sorted(np.concatenate([first, second]), 1.0))
    assert pending.UpdateFinish() and pending.device_updates() == before + 1 and pending.update_counts()["host_updates"] == 0
    assert pending.check() == 0 and twin.update_counts()["host_updates"] == 0
