"""The published clouds as PointCloud2 `data` (RosUtils.cpp:40-63 EigenToPointCloud2, LidarOdometryServer.cpp:240-263 PublishClouds):
kicp_map_pointcloud_f32 on maps that live on the host, and the drop-in's FLOAT32 methods compiling against the headers.  The GPU side is
tests/test_gpu_egress.py."""
import ctypes as C
import os

import numpy as np

import egress_ref as E
import kinematic_icp_amd as K

FLT_MAX = float(np.finfo(np.float32).max)
# values whose narrowing is worth pinning: halfway ties (to even, both ways), float subnormals (kept, and a tie between two of them),
# a tie that rounds to -0.0, signed zeros, the float range's edge (FLT_MAX, the halfway point to 2^128 - rounds to inf -, beyond)
SMALL_EDGES = [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1e-40, -1e-40, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, -(2.0 ** -150),
               2.0 ** -126 * (1 - 2.0 ** -25), -0.0, 0.0, 0.1, 1.0 / 3.0]
HUGE_EDGES = [FLT_MAX, -FLT_MAX, FLT_MAX * (1 + 2.0 ** -25), -FLT_MAX * (1 + 2.0 ** -25), FLT_MAX * (1 + 2.0 ** -26), 1e39, -1e39, 3.0e38]


def pointcloud_f32(m, cap=None):
    """kicp_map_pointcloud_f32 straight through the C-ABI: (rc, total, records as uint32 words)"""
    total = C.c_size_t()
    rc = K.lib().kicp_map_pointcloud_f32(m._h, None, 0, C.byref(total))
    assert rc == 0
    cap = total.value if cap is None else cap
    out = np.full((cap, 3), 0xDEADBEEF, dtype=np.uint32)
    rc = K.lib().kicp_map_pointcloud_f32(m._h, out.ctypes.data if cap else None, cap, C.byref(total))
    return rc, total.value, out


def edge_points(edges, n, spread, rng):
    """n points in distinct voxels (x spread by `spread` per point) whose y and z coordinates cycle through `edges`"""
    e = np.array(edges, dtype=np.float64)
    pts = np.empty((n, 3))
    pts[:, 0] = np.arange(n) * spread + rng.uniform(0, 0.1 * spread, n)
    pts[:, 1] = e[np.arange(n) % e.size]
    pts[:, 2] = e[(np.arange(n) * 7 + 3) % e.size]
    return pts


def edge_maps(n, device=None):
    """a map of small edge values (1 m voxels) and one of values at the float range's edge (voxels of 1e35 m: voxel coordinates stay
    within +-2^20), each filled by one AddPoints call"""
    rng = np.random.default_rng(5)
    small = K.VoxelHashMap(1.0, 1e9, 20, device=device)
    small.AddPoints(edge_points(SMALL_EDGES, n, 3.0, rng))
    huge = K.VoxelHashMap(1e35, 1e300, 20, device=device)
    pts = edge_points(HUGE_EDGES, n, 1e36, rng)
    pts[:, 0] += 4e38  # (x beyond the float range too)
    huge.AddPoints(pts)
    return small, huge


def test_host_map_records_equal_pointcloud_narrowed():
    rng = np.random.default_rng(11)
    m = K.VoxelHashMap(0.5, 50.0, 20)
    for _ in range(3):
        m.Update(rng.uniform(-15, 15, (1500, 3)), rng.uniform(-1, 1, 3))
    rc, total, out = pointcloud_f32(m)
    assert rc == 0 and total == m.num_points() > 1000
    assert np.array_equal(out, E.narrow(m.Pointcloud()))
    assert np.array_equal(m.PointcloudF32().view(np.uint32), E.narrow(m.Pointcloud()))


def test_host_map_empty_and_cap_below_total():
    m = K.VoxelHashMap(1.0, 100.0, 20)
    rc, total, out = pointcloud_f32(m)
    assert (rc, total, out.shape) == (0, 0, (0, 3)) and m.PointcloudF32().shape == (0, 3)
    m.AddPoints(np.random.default_rng(3).uniform(-20, 20, (2000, 3)))
    ref = E.narrow(m.Pointcloud())
    for cap in (1, 5, 1023, len(ref) - 1):
        rc, total, out = pointcloud_f32(m, cap)
        assert rc == 0 and total == len(ref)
        assert np.array_equal(out, ref[:cap]), cap
    # out_xyz NULL with room claimed is an argument error; NULL with cap 0 only reports the count
    total = C.c_size_t()
    assert K.lib().kicp_map_pointcloud_f32(m._h, None, 4, C.byref(total)) < 0
    assert K.lib().kicp_map_pointcloud_f32(m._h, None, 0, C.byref(total)) == 0 and total.value == len(ref)
    m.Clear()
    assert pointcloud_f32(m)[1] == 0


def test_host_map_narrowing_edge_cases():
    small, huge = edge_maps(2000)
    for m in (small, huge):
        rc, total, out = pointcloud_f32(m)
        ref = E.narrow(m.Pointcloud())
        assert rc == 0 and total == len(ref) > 100
        assert np.array_equal(out, ref)
    words = pointcloud_f32(small)[2].ravel()
    assert 0x80000000 in words and 0x00000000 in words                # both zeros, sign kept (-2^-150 ties to -0.0)
    assert ((words & 0x7F800000) == 0).sum() > ((words & 0x7FFFFFFF) == 0).sum()  # subnormals kept, not flushed
    assert 0x3F800000 in words and 0x3F800002 in words                # 1 + 2^-24 -> 1.0, 1 + 3 * 2^-24 -> 1 + 2^-22 (ties to even)
    words = pointcloud_f32(huge)[2].ravel()
    assert 0x7F800000 in words and 0xFF800000 in words and 0x7F7FFFFF in words  # +-inf beyond the range, FLT_MAX below the halfway point


def test_egress_harness_compiles_and_links():
    """tests/cpp/egress_facade_test: KinematicICP::RegisterFrameF32 / RegisterIngestedFrameF32 / LocalMapF32,
    kiss_icp::VoxelHashMap::PointcloudF32 and kicp_bridge::PointCloud2Xyz32 compile and link against libkicp_amd.so"""
    exe = E.build_harness()
    assert os.access(exe, os.X_OK)


def test_record_layout_constants():
    """kicp_bridge::PointCloud2Xyz32 says what EigenToPointCloud2 declares (RosUtils.cpp:45-48): x y z FLOAT32 at 0 4 8, step 12"""
    src = open(os.path.join(E.ROOT, "kinematic_icp_amd", "cpp", "kicp_bridge.hpp")).read()
    block = src[src.index("struct PointCloud2Xyz32"):]
    block = block[:block.index("\n};")]
    for needle in ('{"x", "y", "z"}', "{0, 4, 8}", "KICP_FIELD_FLOAT32", "point_step = 12", "height = 1", "is_bigendian = false"):
        assert needle in block, needle
