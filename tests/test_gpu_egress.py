"""The published clouds as PointCloud2 `data` on the GPU (RosUtils.cpp:40-63 EigenToPointCloud2, LidarOdometryServer.cpp:240-263
PublishClouds): the device map's records (kicp_map_pc.hpp k_pc_records), the frame's (kicp_pre_egress.hpp k_push_frame_f32) and the keypoints',
each compared bit for bit, as uint32 words, with static_cast<float> of the fp64 path's clouds."""
import os
import subprocess

import numpy as np
import pytest

import egress_ref as E
import kinematic_icp_amd as K
from kinematic_icp_amd import synthetic as syn
from oracle import rkicp
from test_egress import edge_maps, pointcloud_f32

pytestmark = pytest.mark.gpu
VOXEL, MAX_RANGE = 0.5, 30.0


def device_map(n_calls=4, n=20000, seed=21):
    """a map filled by bulk updates on the GPU (each call >= 4096 points), the last one with a pose and far-voxel removal"""
    rng = np.random.default_rng(seed)
    m = K.VoxelHashMap(1.0, 60.0, 20, device=0)
    for k in range(n_calls):
        pose = np.array([0.0, 0.0, np.sin(0.1 * k), np.cos(0.1 * k), 2.0 * k, -1.0 * k, 0.1 * k])
        m.Update(rng.uniform(-40, 40, (n, 3)), pose)
    assert bool(K.lib().kicp_map_last_update_on_device(m._h))
    return m


def check_records(m, cap=None):
    ref = E.narrow(m.Pointcloud())
    rc, total, out = pointcloud_f32(m, cap)
    assert rc == 0 and total == len(ref)
    assert np.array_equal(out, ref[: len(out)])
    return len(ref)


def test_gpu_device_map_records_equal_pointcloud_narrowed():
    m = device_map()
    n = check_records(m)
    assert n > 20000
    assert np.array_equal(m.PointcloudF32().view(np.uint32), E.narrow(m.Pointcloud()))
    for cap in (1, 3, 5, 4097, n - 1):  # (fewer records than the map holds, also where the last piece ends mid-unit)
        check_records(m, cap)


def test_gpu_cfg2_size_map_in_several_pieces():
    """about a million points: sixteen pieces of 64 Ki records through four landing slots"""
    rng = np.random.default_rng(9)
    m = K.VoxelHashMap(1.0, 1e6, 20, device=0)
    for _ in range(5):
        m.AddPoints(rng.uniform([0, 0, 0], [120, 120, 12], (260000, 3)))
    assert bool(K.lib().kicp_map_last_update_on_device(m._h))
    n = check_records(m)
    assert n > 800000
    check_records(m, n - 12345)


def test_gpu_after_remove_far_and_clear():
    m = device_map()
    m.RemovePointsFarFromLocation(np.array([5.0, -2.0, 0.0]))
    check_records(m)
    m.Update(np.random.default_rng(4).uniform(-30, 30, (8000, 3)), np.array([0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]))
    check_records(m)
    m.Clear()
    rc, total, out = pointcloud_f32(m)
    assert (rc, total, out.shape) == (0, 0, (0, 3))


def test_gpu_narrowing_edge_cases():
    small, huge = edge_maps(20000, device=0)
    for m in (small, huge):
        assert bool(K.lib().kicp_map_last_update_on_device(m._h))
        check_records(m)
    words = pointcloud_f32(small)[2].ravel()
    assert 0x80000000 in words and ((words & 0x7F800000) == 0).sum() > ((words & 0x7FFFFFFF) == 0).sum()
    words = pointcloud_f32(huge)[2].ravel()
    assert 0x7F800000 in words and 0xFF800000 in words and 0x7F7FFFFF in words


def test_gpu_pending_update_is_collected_first():
    """called right after UpdateDeviceBegin, without UpdateFinish: the records are those of the updated map"""
    m = device_map()
    pre = K.PreSteps(0)
    pre.upload(1, np.random.default_rng(8).uniform(-20, 20, (3000, 3)))
    before = m.num_points()
    m.UpdateDeviceBegin(pre.frame(1), np.array([0.0, 0.0, 0.0, 1.0, 3.0, 0.0, 0.0]))
    got = m.PointcloudF32().view(np.uint32)
    ref = E.narrow(m.Pointcloud())
    assert len(ref) > before and np.array_equal(got, ref)


def test_gpu_presteps_frame_f32_and_keypoints():
    """PreSteps.FrameF32 against Frame on the same cloud; buffer 2's records from either (host copy of the records, or HBM)"""
    ext, frames = E.cloud_drive(2)
    rec, _ = frames[0]
    xyz, st = rec[:, :3].astype(np.float64), rec[:, 3].astype(np.float64) / 0.1
    rel = syn.planar_pose(0.2, 0.0, 0.01)
    pre = K.PreSteps(0)
    counts, frame = pre.Frame(xyz, st, rel, ext, MAX_RANGE, 0.0, True, VOXEL * 0.5, VOXEL * 1.5)
    src = pre.download(2)
    assert np.array_equal(pre.download_f32(2).view(np.uint32), E.narrow(src))  # (after an fp64 frame: narrowed in HBM)
    counts32, frame32 = pre.FrameF32(xyz, st, rel, ext, MAX_RANGE, 0.0, True, VOXEL * 0.5, VOXEL * 1.5)
    assert counts32 == counts and np.array_equal(frame32.view(np.uint32), E.narrow(frame))
    assert np.array_equal(pre.download_f32(2).view(np.uint32), E.narrow(src))
    assert np.array_equal(pre.download(2), src)  # (the fp64 download still gives the doubles)
    counts0, none = pre.FrameF32(xyz, st, rel, ext, MAX_RANGE, 0.0, True, VOXEL * 0.5, VOXEL * 1.5, want_frame=False)
    assert counts0 == counts and none is None
    assert np.array_equal(pre.download_f32(1).view(np.uint32), E.narrow(pre.download(1)))


def run_drive(tmp_path, feed, deskew, dump=None):
    f = tmp_path / "drive.bin"
    if feed == "scan":
        params, ext, frames = syn.make_laser_drive(24)
        E.write_scan_drive(f, params, ext, frames, VOXEL, 25.0, 0.0, deskew)
    else:
        ext, frames = E.cloud_drive(24)
        E.write_cloud_drive(f, ext, frames, VOXEL, MAX_RANGE, 0.0, deskew)
    args = [E.build_harness(), "drive", str(f), feed] + ([str(dump)] if dump else [])
    out = subprocess.check_output(args, text=True, timeout=300).splitlines()
    assert len(out) == 24, out
    for line in out:
        words = line.split()
        assert len(words) == 5, line  # frame k n_frame n_source n_map, and nothing found wrong
        assert int(words[2]) > 0 and int(words[4]) > 0, line
    return ext, frames, out


@pytest.mark.parametrize("deskew", [False, True])
@pytest.mark.parametrize("feed", ["raw", "ahead", "scan", "host"])
def test_gpu_drive_f32_equals_fp64_narrowed(tmp_path, feed, deskew):
    """24 frames through four pipelines (tests/cpp/egress_facade_test drive): the FLOAT32 frame and keypoint bytes equal the fp64
    pipeline's clouds narrowed, the map's bytes its own LocalMap() narrowed (and the fp64 pipeline's points, as sorted records); the
    poses (bit for bit) and map sizes agree with null outputs and with fp64 / FLOAT32 frames alternating"""
    run_drive(tmp_path, feed, deskew)


@pytest.mark.skipif(not rkicp.available(), reason="reference build (oracle/_ref) not present")
def test_gpu_local_map_f32_equals_the_reference_local_map(tmp_path):
    """LocalMapF32 frame by frame against the reference build's own KinematicICP::LocalMap() narrowed - the map the reference node
    publishes.  The order of LocalMap() is the reference's robin_map iteration order, which the backend's table does not reproduce:
    the records are compared as sorted rows."""
    dump = tmp_path / "maps.bin"
    ext, frames, out = run_drive(tmp_path, "host", True, dump)
    maps = E.read_map_dump(dump)
    ref = rkicp.KinematicICP(max_range=MAX_RANGE, min_range=0.0, voxel_size=VOXEL, deskew=True)
    for k, ((rec, delta), ours) in enumerate(zip(frames, maps)):
        t = rec[:, 3].astype(np.float64)
        ref.RegisterFrame(rec[:, :3].astype(np.float64), (t - t.min()) / (t.max() - t.min()), ext, delta)
        theirs = E.narrow(ref.LocalMap())
        assert len(theirs) == len(ours), "frame %d" % k
        a = ours[np.lexsort(ours.T[::-1])]
        b = theirs[np.lexsort(theirs.T[::-1])]
        assert np.array_equal(a, b), "frame %d" % k
