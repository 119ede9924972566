"""The depth view (kicp_view_*): a cube map of depths around the sensor, rendered from one frame, that tells which world points that
frame sees through."""
import ctypes as C

import numpy as np

from ._ffi import Handle, _check, _d, _declare, _dp, _frame_args, _hp, _info, _u8, _u8p, _u64, _u64p, lib


class ViewConfig(C.Structure):
    """kicp_view_config: a cube map of res x res pixels per face; the verdict looks at (2 window + 1)^2 pixels, needs min_rays returns
    among them and a gap of more than margin + margin_per_metre * depth; max_ray bounds the (Chebyshev) depth on both sides"""
    _fields_ = [("res", C.c_uint), ("window", C.c_int), ("min_rays", C.c_uint), ("max_ray", C.c_double), ("margin", C.c_double),
                ("margin_per_metre", C.c_double)]


_ENTRIES = _declare({
    "kicp_view_create": (C.c_int, [C.POINTER(ViewConfig), C.c_int, _hp]),
    "kicp_view_destroy": (None, [C.c_void_p]),
    "kicp_view_info": (C.c_int, [C.c_void_p, C.POINTER(ViewConfig), _dp, _u64p]),
    "kicp_view_render": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _dp, _dp, _u64p]),
    "kicp_view_render_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _dp, _dp, _u64p]),
    "kicp_view_depth": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_size_t]),
    "kicp_view_classify": (C.c_int, [C.c_void_p, _dp, C.c_size_t, _u8p]),
})


class DepthView(Handle):
    """kicp_view: a cube map of depths around the sensor, rendered from ONE frame, that tells which world points that frame sees
    through (include/kicp.h states the exact semantics); VoxelHashMap.RemoveSeenThrough(view) removes them from a map.  It owns its
    device memory; the image stays in HBM until it is asked for."""

    _destroy = "kicp_view_destroy"
    SEEN_THROUGH, IN_RANGE = 1, 2  # bits of a verdict

    def __init__(self, res, window, min_rays, max_ray, margin, margin_per_metre, device=0):
        cfg = ViewConfig(int(res), int(window), int(min_rays), float(max_ray), float(margin), float(margin_per_metre))
        self._create("kicp_view_create", C.byref(cfg), int(device))
        self.device, self.res = device, int(res)
        self._last = np.zeros(2, dtype=np.uint64)

    def info(self):
        """-> dict: the configuration's fields, sensor_world (c of the last frame, NaN before the first) and frames (rendered so far)"""
        return _info("kicp_view_info", self._h, ViewConfig(), sensor_world=np.zeros(3), frames=C.c_ulonglong())

    def render(self, frame, pose, sensor_xyz=(0.0, 0.0, 0.0)):
        """kicp_view_render: the image of one frame of points in the base frame (host memory) at `pose`, the sensor at `sensor_xyz` in the
        base frame -> (points used, points skipped)"""
        _check(lib().kicp_view_render(self._h, *_frame_args(pose, sensor_xyz, frame=frame), _u64(self._last)))
        return self.last_frame()

    def render_device(self, device_frame, pose, sensor_xyz=(0.0, 0.0, 0.0), n=None):
        """kicp_view_render_device: the same for a DeviceFrame (or anything with .ptr and .n) already in HBM"""
        _check(lib().kicp_view_render_device(self._h, *_frame_args(pose, sensor_xyz, device_frame=device_frame, n=n), _u64(self._last)))
        return self.last_frame()

    def last_frame(self):
        """(points used, points skipped) of the last rendered frame"""
        return tuple(int(v) for v in self._last)

    def depth(self):
        """kicp_view_depth -> float32 (6, res, res): [face, w_, u], +inf where no used point fell"""
        out = np.empty((6, self.res, self.res), dtype=np.float32)
        _check(lib().kicp_view_depth(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def classify(self, points):
        """kicp_view_classify: the verdict for world points -> uint8 per point: bit 0 (SEEN_THROUGH), bit 1 (IN_RANGE)"""
        a, p = _d(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        out = np.zeros(a.size // 3, dtype=np.uint8)
        _check(lib().kicp_view_classify(self._h, p if a.size else None, a.size // 3, _u8(out)))
        return out
