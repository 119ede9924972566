"""kiss_icp::VoxelHashMap (kicp_map_*): the map the registration runs against, its updates on the host and on the GPU, its files."""
import ctypes as C
import os

import numpy as np

from ._ffi import Handle, _check, _d, _declare, _dp, _hp, _szp, _u64p, lib

_ENTRIES = _declare({
    "kicp_map_create": (C.c_int, [C.c_double, C.c_double, C.c_uint, _hp]),
    "kicp_map_destroy": (None, [C.c_void_p]),
    "kicp_map_clone": (C.c_int, [C.c_void_p, _hp]),
    "kicp_map_clear": (C.c_int, [C.c_void_p]),
    "kicp_map_empty": (C.c_int, [C.c_void_p]),
    "kicp_map_add_points": (C.c_int, [C.c_void_p, _dp, C.c_size_t]),
    "kicp_map_remove_far": (C.c_int, [C.c_void_p, _dp]),
    "kicp_map_update_origin": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp]),
    "kicp_map_update_pose": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp]),
    "kicp_map_update_pose_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, _dp]),
    "kicp_map_update_pose_device_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, _dp]),
    "kicp_map_update_finish": (C.c_int, [C.c_void_p]),
    "kicp_map_last_update_on_device": (C.c_int, [C.c_void_p]),
    "kicp_map_device_updates": (C.c_ulonglong, [C.c_void_p]),
    "kicp_map_update_counts": (C.c_int, [C.c_void_p, _u64p]),
    "kicp_map_set_device": (C.c_int, [C.c_void_p, C.c_int]),
    "kicp_map_num_points": (C.c_size_t, [C.c_void_p]),
    "kicp_map_num_voxels": (C.c_size_t, [C.c_void_p]),
    "kicp_map_pointcloud": (C.c_size_t, [C.c_void_p, _dp, C.c_size_t]),
    "kicp_map_pointcloud_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _szp]),
    "kicp_map_closest": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_size_t, _dp, _dp]),
    "kicp_map_check": (C.c_size_t, [C.c_void_p]),
    "kicp_map_sync": (C.c_int, [C.c_void_p, C.c_int]),
    "kicp_map_last_upload": (C.c_int, [C.c_void_p, _szp, C.POINTER(C.c_int)]),
    "kicp_map_remove_seen_through": (C.c_int, [C.c_void_p, C.c_void_p, _u64p]),
    "kicp_map_save_pcd": (C.c_int, [C.c_void_p, C.c_char_p]),
    "kicp_map_load_pcd": (C.c_int, [C.c_char_p, C.c_double, C.c_double, C.c_uint, C.c_int, _hp, _szp, _szp]),
    "kicp_map_params": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(C.c_uint)]),
    "kicp_map_device_bytes": (C.c_size_t, [C.c_void_p]),
})


class VoxelHashMap(Handle):
    """kiss_icp::VoxelHashMap: host-authoritative voxel map with an HBM mirror."""

    _destroy = "kicp_map_destroy"

    def __init__(self, voxel_size, max_distance, max_points_per_voxel, device=None):
        """device: preferred GPU for bulk insertions (AddPoints / Update with >= 4096 points run there); None = on the host."""
        self.voxel_size_, self.max_distance_, self.max_points_per_voxel_ = voxel_size, max_distance, max_points_per_voxel
        self._create("kicp_map_create", voxel_size, max_distance, max_points_per_voxel)
        if device is not None:
            self.set_device(device)

    def set_device(self, device):
        _check(lib().kicp_map_set_device(self._h, -1 if device is None else int(device)))

    def copy(self):
        """VoxelHashMap(const VoxelHashMap&): a deep copy of the newest state."""
        c = VoxelHashMap._from("kicp_map_clone", self._h)
        c.voxel_size_, c.max_distance_, c.max_points_per_voxel_ = self.voxel_size_, self.max_distance_, self.max_points_per_voxel_
        return c

    def save_pcd(self, path):
        """The map as a PCD v0.7 file, DATA binary (kicp_map_save_pcd): Pointcloud() in its order plus a comment line with the three
        parameters.  A pending map update's error is raised here."""
        _check(lib().kicp_map_save_pcd(self._h, os.fsencode(path)))

    @staticmethod
    def load_pcd(path, voxel_size=0.0, max_distance=0.0, max_points_per_voxel=0, device=None):
        """A new map from a PCD file (kicp_map_load_pcd), its points inserted in file order - on `device` (bulk insertion) or, with None,
        on the host.  voxel_size <= 0: the parameters come from the file's `# kicp_map` line.  The new map's `points_read` and
        `points_dropped` tell how many rows the file held and how many of them were not finite."""
        read, dropped = C.c_size_t(), C.c_size_t()
        m = VoxelHashMap._from("kicp_map_load_pcd", os.fsencode(path), float(voxel_size), float(max_distance), int(max_points_per_voxel),
                               -1 if device is None else int(device), tail=(C.byref(read), C.byref(dropped)))
        vs, md, cap = C.c_double(), C.c_double(), C.c_uint()
        _check(lib().kicp_map_params(m._h, C.byref(vs), C.byref(md), C.byref(cap)))
        m.voxel_size_, m.max_distance_, m.max_points_per_voxel_ = vs.value, md.value, cap.value
        m.points_read, m.points_dropped = read.value, dropped.value
        return m

    def Clear(self):
        _check(lib().kicp_map_clear(self._h))

    def Empty(self):
        return bool(lib().kicp_map_empty(self._h))

    def AddPoints(self, points):
        a, p = _d(points)
        _check(lib().kicp_map_add_points(self._h, p, a.size // 3))

    def RemovePointsFarFromLocation(self, origin):
        _, p = _d(origin)
        _check(lib().kicp_map_remove_far(self._h, p))

    def Update(self, points, pose_or_origin):
        a, p = _d(points)
        b, q = _d(pose_or_origin)
        if b.size == 7:
            _check(lib().kicp_map_update_pose(self._h, p, a.size // 3, q))
        elif b.size == 3:
            _check(lib().kicp_map_update_origin(self._h, p, a.size // 3, q))
        else:
            raise ValueError("Update expects a 7-vector pose or a 3-vector origin")

    def UpdateDevice(self, device_frame, pose):
        """Update(points, pose) with the points already in HBM (DeviceFrame / PreSteps.frame); returns True if it ran on
        the GPU (table and pool growth included), False if the host map took it over: no points, or a map that holds or
        meets a voxel beyond +-2^20 voxels from the origin."""
        _, q = _d(pose)
        _check(lib().kicp_map_update_pose_device(self._h, device_frame.device, device_frame.ptr, device_frame.n, q))
        return bool(lib().kicp_map_last_update_on_device(self._h))

    def UpdateDeviceBegin(self, device_frame, pose):
        """kicp_map_update_pose_device_begin: the update's kernels are queued, nothing is waited for (UpdateFinish, or any other
        call on the map, collects it); the frame must stay alive and unchanged until then"""
        _, q = _d(pose)
        _check(lib().kicp_map_update_pose_device_begin(self._h, device_frame.device, device_frame.ptr, device_frame.n, q))

    def UpdateFinish(self):
        _check(lib().kicp_map_update_finish(self._h))
        return bool(lib().kicp_map_last_update_on_device(self._h))

    def RemoveSeenThrough(self, view):
        """kicp_map_remove_seen_through: remove every map point the frame in `view` (a DepthView) sees through -> (points in range, points
        removed, voxels that lost at least one point, voxels erased).  A pending map update is collected first."""
        out = (C.c_ulonglong * 4)()
        _check(lib().kicp_map_remove_seen_through(self._h, view._h, out))
        return tuple(int(v) for v in out)

    def device_updates(self):
        """Updates that ran on the GPU and have been collected (kicp_map_device_updates); a pending one stays pending."""
        return lib().kicp_map_device_updates(self._h)

    UPDATE_COUNTS = ("one_queue", "staged", "second_claims", "rehashes", "pool_growths", "apply_wave", "apply_thread", "wide_scans",
                     "host_updates", "deferred", "touched", "record_pieces")

    def update_counts(self):
        """Which way this map's updates went so far (kicp_map_update_counts, include/kicp.h): a dict of the twelve host-side
        counters; reads no device state and does not collect a pending update.  "record_pieces": pieces of PointcloudF32 /
        kicp_map_pointcloud_f32 calls that the device announced and the host copied (the host path and the fallback leave it alone)."""
        out = (C.c_ulonglong * 12)()
        _check(lib().kicp_map_update_counts(self._h, out))
        return dict(zip(self.UPDATE_COUNTS, out))

    def num_points(self):
        return lib().kicp_map_num_points(self._h)

    def num_voxels(self):
        return lib().kicp_map_num_voxels(self._h)

    def Pointcloud(self):
        n = self.num_points()
        out = np.empty((n, 3), dtype=np.float64)
        lib().kicp_map_pointcloud(self._h, out.ctypes.data_as(_dp), n)
        return out

    def PointcloudF32(self):
        """Pointcloud() as the published map's PointCloud2 records (kicp_map_pointcloud_f32): (n, 3) float32, static_cast<float> of
        Pointcloud(), narrowed on the GPU where the map lives there.  A pending map update's error is raised here."""
        n = C.c_size_t()
        _check(lib().kicp_map_pointcloud_f32(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), dtype=np.float32)
        _check(lib().kicp_map_pointcloud_f32(self._h, out.ctypes.data if n.value else None, n.value, C.byref(n)))
        return out

    def GetClosestNeighbor(self, queries, device=0):
        """Batch form of GetClosestNeighbor: (N,3) queries -> ((N,3) neighbours, (N,) distances)."""
        a, p = _d(queries)
        n = a.size // 3
        nn = np.empty((n, 3), dtype=np.float64)
        d = np.empty(n, dtype=np.float64)
        _check(lib().kicp_map_closest(self._h, device, p, n, nn.ctypes.data_as(_dp), d.ctypes.data_as(_dp)))
        return nn, d

    def check(self):
        """Number of violated table invariants on the host copy (0 = consistent); debug aid."""
        return lib().kicp_map_check(self._h)

    def sync(self, device=0):
        _check(lib().kicp_map_sync(self._h, device))

    def device_bytes(self):
        return lib().kicp_map_device_bytes(self._h)

    def last_upload(self):
        """(bytes sent by the last mirror upload, True if it was a full re-send rather than a delta)."""
        b, f = C.c_size_t(), C.c_int()
        _check(lib().kicp_map_last_upload(self._h, C.byref(b), C.byref(f)))
        return b.value, bool(f.value)
