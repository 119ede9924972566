"""The pipeline's pre-steps on the GPU (kicp_pre_*): wire-format ingest, deskew and crop, the two voxel downsamples, and the numbered
device buffers their results live in."""
import ctypes as C

import numpy as np

from ._ffi import Handle, KicpError, _check, _d, _declare, _dp, _hp, _szp, lib
from .device import DeviceFrame


class CloudLayout(C.Structure):
    """kicp_cloud_layout (include/kicp.h): where x, y, z and the per-point stamp sit inside a PointCloud2 record."""
    _fields_ = [("point_step", C.c_uint), ("offset_x", C.c_uint), ("offset_y", C.c_uint), ("offset_z", C.c_uint),
                ("stamp_datatype", C.c_int), ("offset_stamp", C.c_uint)]


FIELD_UINT32, FIELD_FLOAT32, FIELD_FLOAT64 = 6, 7, 8  # sensor_msgs::msg::PointField datatype codes


class LaserScan(C.Structure):
    """kicp_laser_scan (include/kicp.h): the sensor_msgs::msg::LaserScan fields laser_geometry's projectLaser reads."""
    _fields_ = [("angle_min", C.c_float), ("angle_max", C.c_float), ("angle_increment", C.c_float), ("time_increment", C.c_float),
                ("range_min", C.c_float), ("range_max", C.c_float)]


_vp, _f64, _sz = C.c_void_p, C.c_double, C.c_size_t
# what the four kicp_pre_frame* entries take in their middle: relative motion, lidar to base, max range, min range, deskew, voxel a, voxel b
_frame_mid = [_dp, _dp, _f64, _f64, C.c_int, _f64, _f64]

_ENTRIES = _declare({
    "kicp_pre_create": (C.c_int, [C.c_int, _hp]),
    "kicp_pre_destroy": (None, [_vp]),
    "kicp_pre_preprocess": (C.c_int, [_vp, _dp, _sz, _dp, _sz, _dp, _dp, _f64, _f64, C.c_int, C.c_int, _szp]),
    "kicp_pre_ingest": (C.c_int, [_vp, _vp, _sz, _vp, _dp, _dp, _dp]),
    "kicp_pre_ingest_ahead": (C.c_int, [_vp, _vp, _sz, _vp, _dp]),
    "kicp_pre_ingest_scan": (C.c_int, [_vp, _vp, _sz, _vp, _f64, _dp, _dp]),
    "kicp_pre_ahead_hits": (C.c_ulonglong, [_vp]),
    "kicp_pre_set_option": (C.c_int, [_vp, C.c_char_p, _f64]),
    "kicp_pre_get_option": (_f64, [_vp, C.c_char_p]),
    "kicp_pre_preprocess_ingested": (C.c_int, [_vp, _dp, _dp, _f64, _f64, C.c_int, C.c_int, _szp]),
    "kicp_pre_ingested": (C.c_int, [_vp, _dp, _dp, _sz, _szp, C.POINTER(C.c_int)]),
    "kicp_pre_frame": (C.c_int, [_vp, _dp, _sz, _dp, _sz] + _frame_mid + [_dp, _sz, _szp]),
    "kicp_pre_frame_ingested": (C.c_int, [_vp] + _frame_mid + [_dp, _sz, _szp]),
    "kicp_pre_frame_f32": (C.c_int, [_vp, _dp, _sz, _dp, _sz] + _frame_mid + [_vp, _sz, _szp]),
    "kicp_pre_frame_ingested_f32": (C.c_int, [_vp] + _frame_mid + [_vp, _sz, _szp]),
    "kicp_pre_ingested_count": (_sz, [_vp]),
    "kicp_pre_voxel_downsample": (C.c_int, [_vp, C.c_int, _f64, C.c_int, _szp]),
    "kicp_pre_last_max_probe": (C.c_uint, [_vp]),
    "kicp_pre_set_probe_limit": (C.c_int, [_vp, C.c_uint]),
    "kicp_pre_upload": (C.c_int, [_vp, C.c_int, _dp, _sz]),
    "kicp_pre_download": (C.c_int, [_vp, C.c_int, _dp, _sz, _szp]),
    "kicp_pre_download_f32": (C.c_int, [_vp, C.c_int, _vp, _sz, _szp]),
    "kicp_pre_download_begin": (C.c_int, [_vp, C.c_int]),
    "kicp_pre_download_begin_into": (C.c_int, [_vp, C.c_int, _dp, _sz]),
    "kicp_pre_download_finish": (C.c_int, [_vp, C.c_int, _dp, _sz, _szp]),
    "kicp_pre_device_ptr": (_vp, [_vp, C.c_int, _szp]),
})


class PreSteps(Handle):
    """The pipeline's pre-steps on the GPU: kiss_icp::Preprocessor::Preprocess + transform_points, kiss_icp::VoxelDownsample
    (pipeline/KinematicICP.cpp:54-62).  Results live in numbered device buffers; frame(b) wraps one for ComputeRobotMotion."""

    _destroy = "kicp_pre_destroy"

    def __init__(self, device=0):
        self._create("kicp_pre_create", device)
        self.device = device

    def set_probe_limit(self, limit):
        """probe length at which the reference's tsl::robin_map grows its table (128: robin-map 0.6.x, default; 8192: 1.x)"""
        _check(lib().kicp_pre_set_probe_limit(self._h, int(limit)))

    def last_max_probe(self):
        """Largest robin-hood displacement the last VoxelDownsample's replay saw (kicp_pre_last_max_probe)."""
        return int(lib().kicp_pre_last_max_probe(self._h))

    def Preprocess(self, frame, timestamps, relative_motion, lidar_to_base, max_range, min_range, deskew, dst=0):
        a, p = _d(frame)
        t, tp = _d(timestamps if timestamps is not None else np.zeros(0))
        _, r = _d(relative_motion)
        _, e = _d(lidar_to_base)
        n = C.c_size_t()
        _check(lib().kicp_pre_preprocess(self._h, p, a.size // 3, tp, t.size, r, e, max_range, min_range, int(deskew), dst, C.byref(n)))
        return n.value

    def Ingest(self, raw, n_points, point_step, offset_x, offset_y, offset_z, stamp_datatype=0, offset_stamp=0, sensor_pose=None):
        """PointCloud2 wire-format ingest (RosUtils.cpp:30-39 PointCloud2ToEigen + TimeStampHandler.cpp:57-128): ships the raw
        message bytes and decodes them on the GPU.  Returns (min_stamp, max_stamp) in seconds (0, 0 without a stamp field)."""
        buf = np.ascontiguousarray(np.frombuffer(raw, dtype=np.uint8))
        layout = CloudLayout(point_step, offset_x, offset_y, offset_z, stamp_datatype, offset_stamp)
        q = None if sensor_pose is None else _d(sensor_pose)[1]
        lo, hi = C.c_double(), C.c_double()
        _check(lib().kicp_pre_ingest(self._h, buf.ctypes.data if buf.size else None, n_points, C.byref(layout), q, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def IngestScan(self, ranges, angle_min, angle_max, angle_increment, time_increment, range_min, range_max, range_cutoff=-1.0):
        """2-D LaserScan ingest (kicp_pre_ingest_scan): laser_geometry's projectLaser(scan, cloud, range_cutoff, Timestamp) of the
        2-D node (online_node.cpp:44-58) on the GPU, then what Ingest does with the projected cloud.  `ranges`: msg.ranges (float32).
        Returns (min_stamp, max_stamp) of the kept beams in seconds (0, 0 when none was kept)."""
        r = np.ascontiguousarray(ranges, dtype=np.float32).ravel()
        scan = LaserScan(angle_min, angle_max, angle_increment, time_increment, range_min, range_max)
        lo, hi = C.c_double(), C.c_double()
        _check(lib().kicp_pre_ingest_scan(self._h, r.ctypes.data if r.size else None, r.size, C.byref(scan), float(range_cutoff),
                                          C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def IngestAhead(self, raw, n_points, point_step, offset_x, offset_y, offset_z, stamp_datatype=0, offset_stamp=0, sensor_pose=None):
        """kicp_pre_ingest_ahead: announce the NEXT message (`raw` must be a buffer whose memory the later Ingest call passes again - a
        numpy uint8 array); it is uploaded and decoded by the next Frame() call on the current one."""
        buf = np.ascontiguousarray(np.frombuffer(raw, dtype=np.uint8))
        layout = CloudLayout(point_step, offset_x, offset_y, offset_z, stamp_datatype, offset_stamp)
        q = None if sensor_pose is None else _d(sensor_pose)[1]
        self._ahead_keep = (buf, raw)  # (borrowed by the backend until the Ingest call for the same bytes)
        _check(lib().kicp_pre_ingest_ahead(self._h, buf.ctypes.data if buf.size else None, n_points, C.byref(layout), q))

    def set_option(self, name, value):
        _check(lib().kicp_pre_set_option(self._h, name.encode(), float(value)))

    def get_option(self, name):
        return float(lib().kicp_pre_get_option(self._h, name.encode()))

    def ahead_hits(self):
        return int(lib().kicp_pre_ahead_hits(self._h))

    def PreprocessIngested(self, relative_motion, lidar_to_base, max_range, min_range, deskew, dst=0):
        _, r = _d(relative_motion)
        _, e = _d(lidar_to_base)
        n = C.c_size_t()
        _check(lib().kicp_pre_preprocess_ingested(self._h, r, e, max_range, min_range, int(deskew), dst, C.byref(n)))
        return n.value

    def ingested(self):
        """(xyz (n,3) fp64, normalised stamps (n,) or None): what PointCloud2ToEigen / ProcessTimestamps hand to RegisterFrame."""
        n, has = C.c_size_t(), C.c_int()
        _check(lib().kicp_pre_ingested(self._h, None, None, 0, C.byref(n), C.byref(has)))
        xyz, st = np.empty((n.value, 3)), np.empty(n.value)
        _check(lib().kicp_pre_ingested(self._h, xyz.ctypes.data_as(_dp), st.ctypes.data_as(_dp), n.value, C.byref(n), C.byref(has)))
        return xyz, (st if has.value else None)

    def _frame(self, dtype, entry, entry_ingested, frame, timestamps, relative_motion, lidar_to_base, max_range, min_range, deskew, voxel_a, voxel_b,
               want_frame):
        """Frame / FrameF32: the chained pre-steps through `entry` (or `entry_ingested`, frame=None), the preprocessed frame landing in
        an (n, 3) array of `dtype`."""
        _, r = _d(relative_motion)
        _, e = _d(lidar_to_base)
        counts = (C.c_size_t * 3)()
        f64 = dtype is np.float64
        if frame is None:
            n_in = lib().kicp_pre_ingested_count(self._h)
        else:
            a, p = _d(frame)
            t, tp = _d(timestamps if timestamps is not None else np.zeros(0))
            n_in = a.size // 3
        out = np.empty((n_in, 3), dtype=dtype) if want_frame else None
        landing = (out.ctypes.data_as(_dp) if f64 else out.ctypes.data) if want_frame and n_in else None
        tail = (r, e, max_range, min_range, int(deskew), voxel_a, voxel_b, landing, n_in, counts)
        rc = entry_ingested(self._h, *tail) if frame is None else entry(self._h, p, n_in, tp, t.size, *tail)
        if rc < 0:
            message = lib().kicp_last_error().decode(errors="replace")
            if want_frame and n_in:  # the backend's helper thread may hold a pointer into `out`: collect (and drop) the download before the array can go
                lib().kicp_pre_download_finish(self._h, 0, None, 0, None)
            raise KicpError(rc, message)
        self.last_status = rc
        if want_frame and n_in:
            n = C.c_size_t()  # (FLOAT32 records land in `out` only: collected with NULL)
            _check(lib().kicp_pre_download_finish(self._h, 0, landing if f64 else None, n_in if f64 else 0, C.byref(n)))
            out = out[:counts[0]]
        return [int(c) for c in counts], out

    def Frame(self, frame, timestamps, relative_motion, lidar_to_base, max_range, min_range, deskew, voxel_a, voxel_b, want_frame=True):
        """kicp_pre_frame / kicp_pre_frame_ingested (frame=None: the ingested cloud): Preprocess + the two downsamples behind one
        synchronisation.  Returns (counts, preprocessed frame or None)."""
        return self._frame(np.float64, lib().kicp_pre_frame, lib().kicp_pre_frame_ingested, frame, timestamps, relative_motion, lidar_to_base, max_range,
                           min_range, deskew, voxel_a, voxel_b, want_frame)

    def FrameF32(self, frame, timestamps, relative_motion, lidar_to_base, max_range, min_range, deskew, voxel_a, voxel_b, want_frame=True):
        """kicp_pre_frame_f32 / kicp_pre_frame_ingested_f32: Frame() with the preprocessed frame returned as PointCloud2 records, (n, 3)
        float32 narrowed on the GPU (want_frame=False: nothing is pushed).  Returns (counts, records or None); download_f32(2) then
        reads the keypoints' records."""
        return self._frame(np.float32, lib().kicp_pre_frame_f32, lib().kicp_pre_frame_ingested_f32, frame, timestamps, relative_motion, lidar_to_base,
                           max_range, min_range, deskew, voxel_a, voxel_b, want_frame)

    def download_f32(self, buffer):
        """kicp_pre_download_f32: a buffer as PointCloud2 records, (n, 3) float32"""
        n = C.c_size_t()
        _check(lib().kicp_pre_download_f32(self._h, buffer, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), dtype=np.float32)
        _check(lib().kicp_pre_download_f32(self._h, buffer, out.ctypes.data if n.value else None, n.value, C.byref(n)))
        return out

    def VoxelDownsample(self, src, voxel_size, dst):
        n = C.c_size_t()
        self.last_status = _check(lib().kicp_pre_voxel_downsample(self._h, src, voxel_size, dst, C.byref(n)))  # KICP_WARN_TABLE_ORDER: see kicp.h
        return n.value

    def upload(self, buffer, points):
        a, p = _d(points)
        _check(lib().kicp_pre_upload(self._h, buffer, p, a.size // 3))

    def download(self, buffer):
        n = C.c_size_t()
        _check(lib().kicp_pre_download(self._h, buffer, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), dtype=np.float64)
        _check(lib().kicp_pre_download(self._h, buffer, out.ctypes.data_as(_dp), n.value, C.byref(n)))
        return out

    def download_begin(self, buffer):
        """Start copying a buffer to the host in the background; collect it with download_finish."""
        _check(lib().kicp_pre_download_begin(self._h, buffer))

    def download_finish(self, buffer):
        n = C.c_size_t()
        _check(lib().kicp_pre_download(self._h, buffer, None, 0, C.byref(n)))  # (size only)
        out = np.empty((n.value, 3), dtype=np.float64)
        _check(lib().kicp_pre_download_finish(self._h, buffer, out.ctypes.data_as(_dp), n.value, C.byref(n)))
        return out[:n.value]

    def frame(self, buffer):
        """A DeviceFrame view of a buffer (no copy; valid until the buffer is overwritten)."""
        n = C.c_size_t()
        ptr = lib().kicp_pre_device_ptr(self._h, buffer, C.byref(n))
        return DeviceFrame._borrow(ptr, n.value, self.device)
