"""What the device-side map update is compared with: the sequential oracle and - where oracle/_ref is present - the reference
build's own kiss_icp::VoxelHashMap, driven in lock step (`Oracles`), and a comparison that sees the ORDER of the points inside every
bucket (`assert_same_buckets`), not only the clouds as sets.  No GPU import: tests/test_mapdev_scenes.py uses it on the CPU."""
import numpy as np

from checkers import okicp, ref_available, rkicp


def bucket_sorted(pc, vs):
    """The cloud grouped by voxel with each voxel's points left in the order the map lists them: a STABLE sort by the voxel key
    floor(p / vs) - the same IEEE division as the reference's PointToVoxel.  Two maps that hold the same voxels, the same points in each
    and the same order inside each bucket give the same array row for row, however their tables order the voxels."""
    pc = np.asarray(pc, dtype=np.float64).reshape(-1, 3)
    key = np.floor(pc / vs)
    return pc[np.lexsort((key[:, 2], key[:, 1], key[:, 0]))]  # (lexsort is stable)


class Oracles:
    """okicp.VoxelHashMap and, where available, rkicp.VoxelHashMap behind one interface; every answer is given by both and must agree
    (clouds bucket by bucket in order, neighbours bit for bit) before anything is compared with it."""

    def __init__(self, vs, max_distance, cap):
        self.vs = vs
        self.o = okicp.VoxelHashMap(vs, max_distance, cap)
        self.r = rkicp.VoxelHashMap(vs, max_distance, cap) if ref_available() else None

    def _both(self):
        return [self.o] if self.r is None else [self.o, self.r]

    def AddPoints(self, pts):
        for m in self._both():
            m.AddPoints(pts)

    def Update(self, pts, pose_or_origin):
        for m in self._both():
            m.Update(pts, pose_or_origin)

    def RemovePointsFarFromLocation(self, origin):
        for m in self._both():
            m.RemovePointsFarFromLocation(origin)

    def Clear(self):
        for m in self._both():
            m.Clear()

    def num_points(self):
        n = self.o.num_points()
        assert self.r is None or self.r.num_points() == n
        return n

    def num_voxels(self):
        n = self.o.num_voxels()
        assert self.r is None or self.r.num_voxels() == n
        return n

    def buckets(self):
        """bucket_sorted(Pointcloud()), the oracle's and the reference build's agreeing row for row"""
        b = bucket_sorted(self.o.Pointcloud(), self.vs)
        if self.r is not None:
            np.testing.assert_array_equal(b, bucket_sorted(self.r.Pointcloud(), self.vs), err_msg="oracle and reference build disagree")
        return b

    def GetClosestNeighbor(self, q):
        nn, d = self.o.GetClosestNeighbor(q)
        if self.r is not None:
            nn_r, d_r = self.r.GetClosestNeighbor(q)
            assert np.array_equal(nn, nn_r) and np.array_equal(d, d_r), "oracle and reference build disagree"
        return nn, d

    def verdicts(self, pts):
        """AddPoints one point at a time -> which of them the oracle kept (bool per point)"""
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        kept = np.zeros(len(pts), dtype=bool)
        before = self.o.num_points()
        for i in range(len(pts)):
            self.o.AddPoints(pts[i:i + 1])
            after = self.o.num_points()
            kept[i], before = after != before, after
        if self.r is not None:
            self.r.AddPoints(pts)
            assert self.r.num_points() == before
        return kept


def assert_same_buckets(gmap, omap, vs, msg=""):
    """The device-maintained map `gmap` against `omap` (an Oracles): the same voxels, the same points in each, the same order inside each
    bucket.  First on the cloud as the GPU gathers it while the HBM copy is the newer one, then - check() == 0 has forced the download -
    on the host copy, which must list the very same array."""
    want = omap.buckets()
    pc_device = gmap.Pointcloud()
    assert len(pc_device) == len(want), "%s: %d points, the oracle holds %d" % (msg, len(pc_device), len(want))
    np.testing.assert_array_equal(bucket_sorted(pc_device, vs), want, err_msg=msg)
    assert gmap.check() == 0, msg
    np.testing.assert_array_equal(gmap.Pointcloud(), pc_device, err_msg=msg + " (host copy after the download)")
