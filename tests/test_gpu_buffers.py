"""One handle across sizes that make every buffer behind it grow, be reused, and grow again (the owning buffer types of
csrc/kicp_internal.hpp): whatever a handle computed after its buffers were replaced equals, bit for bit, what a fresh handle
computes - and what the oracle computes where an existing test shows how."""
import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import sort_rows
from kinematic_icp_amd import synthetic as syn
from checkers import okicp

pytestmark = pytest.mark.gpu


def test_presteps_handle_grows_and_is_reused():
    """200 points leave room for 1 274 (n + n / 4 + 1024): 3 000 grow every buffer, 200 reuse them, 9 000 grow them again."""
    rng = np.random.default_rng(3)
    ext = np.array([0.0, 0.0, np.sin(0.05), np.cos(0.05), 0.3, 0.1, 0.9])
    rel = syn.planar_pose(0.6, 0.05, 0.04)
    pre = K.PreSteps()
    for n in (200, 3000, 200, 9000):
        frame = rng.uniform(-20.0, 20.0, (n, 3)) * np.array([1.0, 1.0, 0.1])
        ts = np.linspace(0.0, 1.0, n)
        fresh = K.PreSteps()
        outs = []
        for h in (pre, fresh):
            kept = h.Preprocess(frame, ts, rel, ext, 25.0, 2.0, 1, dst=0)
            a = h.download(0)
            down = h.VoxelDownsample(0, 0.5, 1)
            outs.append((kept, a, down, h.download(1)))
        (kept, a, down, b), (kept_f, a_f, down_f, b_f) = outs
        assert 0 < down <= kept < n, n  # (the crop and the downsample both removed something)
        assert (kept, down) == (kept_f, down_f), n
        assert np.array_equal(a, a_f) and np.array_equal(b, b_f), n
        np.testing.assert_array_equal(b, okicp.voxel_downsample(a, 0.5))


def test_registration_handle_grows_and_is_reused():
    """400-point scans take the small path (command line, rows), 30 000 and 60 000 points the generic kernels (frame, rows,
    partials with their tickets and accumulators): each size after the others on one handle."""
    rng = np.random.default_rng(5)
    pts = rng.normal(0, 8, (20000, 3)) * np.array([1, 1, 0.2])
    gmap = K.VoxelHashMap(1.0, 40.0, 20)
    gmap.AddPoints(pts)
    last, rel = syn.planar_pose(0.3, -0.2, 0.02), syn.planar_pose(0.05, 0.0, 0.004)
    reg = K.KinematicRegistration()
    for n in (400, 30000, 400, 60000):
        scan = pts[rng.integers(0, len(pts), n)] + rng.normal(0, 0.05, (n, 3))
        scan = okicp.se3_act(okicp.se3_inverse(syn.pose_mul(last, rel)), scan)
        fresh = K.KinematicRegistration()
        a = reg.ComputeRobotMotion(scan, gmap, last, rel, 1.0)
        b = fresh.ComputeRobotMotion(scan, gmap, last, rel, 1.0)
        assert (reg.get_option("small_active") != 0.0) == (n == 400), n
        assert fresh.get_option("small_active") == reg.get_option("small_active"), n
        assert np.array_equal(a, b) and np.all(np.isfinite(a)), n
        assert reg.last_stats.iterations == fresh.last_stats.iterations >= 1, n


def _same_map(g, o):
    assert (g.num_points(), g.num_voxels()) == (o.num_points(), o.num_voxels())
    np.testing.assert_array_equal(sort_rows(g.Pointcloud()), sort_rows(o.Pointcloud()))


def test_map_mirror_grows_rehashes_and_is_dropped():
    rng = np.random.default_rng(9)
    g, o = K.VoxelHashMap(1.0, 60.0, 20), okicp.VoxelHashMap(1.0, 60.0, 20)
    first = rng.normal(0, 3, (100, 3))
    g.UpdateDevice(K.DeviceFrame(first), syn.IDENTITY), o.Update(first, syn.IDENTITY)
    on_device = 0
    for k in range(5):  # 4 000 points at shifted poses: the pools grow and the table is re-hashed on the device
        chunk = rng.normal(0, 6, (4000, 3)) * np.array([1, 1, 0.2])
        pose = syn.planar_pose(4.0 * (k + 1), -2.0 * k, 0.3 * k)
        on_device += int(g.UpdateDevice(K.DeviceFrame(chunk), pose))
        o.Update(chunk, pose)
    assert on_device == 5
    _same_map(g, o)  # (gathered on the device: the HBM copy is the newer one)
    twin = g.copy()  # ... of which the copy is taken
    _same_map(twin, o)
    assert g.check() == 0 and twin.check() == 0
    _same_map(g, o)
    before = sort_rows(o.Pointcloud())
    g.Clear(), o.Clear()
    g.UpdateDevice(K.DeviceFrame(first), syn.IDENTITY), o.Update(first, syn.IDENTITY)
    _same_map(g, o)
    assert g.check() == 0
    np.testing.assert_array_equal(sort_rows(twin.Pointcloud()), before)  # the copy kept its own state
    if K.device_count() > 1:  # the mirror moves to another device: the first one's buffers are dropped
        g.sync(0), g.sync(1)
        q = rng.normal(0, 3, (200, 3))
        nn_g, d_g = g.GetClosestNeighbor(q, device=1)
        nn_o, d_o = o.GetClosestNeighbor(q)
        assert np.array_equal(nn_g, nn_o) and np.array_equal(d_g, d_o)
        _same_map(g, o)

