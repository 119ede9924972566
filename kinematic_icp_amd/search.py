"""Whole-map relocalisation's search space (kicp_occ_*, kicp_search_*): the occupancy pyramid of a map and the window of planar poses
that KinematicRegistration.SearchPoses walks over it."""
import ctypes as C

import numpy as np

from ._ffi import Handle, _check, _d, _declare, _dp, _hp, _intp, _szp, _u32, _u32p, _u64p, lib


class SearchWindow(C.Structure):
    """kicp_search_window: node (j, ix, iy) is the planar pose at (x0 + ix cell, y0 + iy cell, z) with yaw yaw0 + j yaw_step; its index
    is (j * ny + iy) * nx + ix"""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("z", C.c_double), ("nx", C.c_uint), ("ny", C.c_uint), ("yaw0", C.c_double),
                ("yaw_step", C.c_double), ("nyaw", C.c_uint)]

    @property
    def nodes(self):
        return int(self.nx) * int(self.ny) * int(self.nyaw)


_ENTRIES = _declare({
    "kicp_occ_build": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, _hp]),
    "kicp_occ_destroy": (None, [C.c_void_p]),
    "kicp_occ_info": (C.c_int, [C.c_void_p, _dp, _intp, _dp, _intp, _intp, _u64p]),
    "kicp_occ_level": (C.c_int, [C.c_void_p, C.c_int, _u32p, C.c_size_t, _szp]),
    "kicp_search_yaws": (C.c_int, [C.POINTER(SearchWindow), _dp]),
    "kicp_search_window_around": (C.c_int, [C.c_void_p, _dp, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(SearchWindow)]),
})


def search_yaws(window):
    """kicp_search_yaws: the (nyaw, 2) table of (cos, sin) the node scores are computed from - the very doubles the device uses"""
    out = np.zeros((window.nyaw, 2), dtype=np.float64)
    _check(lib().kicp_search_yaws(C.byref(window), out.ctypes.data_as(_dp)))
    return out


def search_window_around(occ, center_xy, half_x, half_y, z, yaw_step):
    """kicp_search_window_around: the window of nodes within the half extents of center_xy (rounded down to whole cells of the pyramid)
    over the full circle of yaws; half extents <= 0 (center_xy may be None): the pyramid's whole x-y footprint -> SearchWindow"""
    w = SearchWindow()
    center, c = (None, None) if center_xy is None else _d(np.asarray(center_xy, dtype=np.float64).reshape(2))  # (`center` keeps the array alive)
    _check(lib().kicp_search_window_around(occ._h, c, float(half_x), float(half_y), float(z), float(yaw_step), C.byref(w)))
    return w


class OccupancyPyramid(Handle):
    """kicp_occ: a SNAPSHOT of a map as an occupancy grid of `cell` metres (every point's cell and those within `dilate` of it) and
    `levels` max-pooled levels above it (include/kicp.h).  It owns its device memory and does not follow later updates of the map."""

    _destroy = "kicp_occ_destroy"

    def __init__(self, voxel_map, cell, dilate=1, levels=4, device=0):
        self._create("kicp_occ_build", voxel_map._h, int(device), float(cell), int(dilate), int(levels))
        self.device = device

    @classmethod
    def build(cls, voxel_map, cell, dilate=1, levels=4, device=0):
        """kicp_occ_build, spelled as the C-ABI spells it: the same as calling the class"""
        return cls(voxel_map, cell, dilate, levels, device)

    def info(self):
        """-> dict: min[3], dims[3], cell, dilate, levels, set_cells (level 0)"""
        mn, dims = np.zeros(3, dtype=np.float64), (C.c_int * 3)()
        cell, dilate, levels, set_cells = C.c_double(), C.c_int(), C.c_int(), C.c_ulonglong()
        _check(lib().kicp_occ_info(self._h, mn.ctypes.data_as(_dp), dims, C.byref(cell), C.byref(dilate), C.byref(levels), C.byref(set_cells)))
        return {"min": mn, "dims": np.array(list(dims), dtype=np.int64), "cell": cell.value, "dilate": dilate.value, "levels": levels.value,
                "set_cells": set_cells.value}

    def level(self, level):
        """one level as uint32 words shaped (dims z, dims y, words per row): cell (x, y, z) is bit x & 31 of [z, y, x >> 5]"""
        total = C.c_size_t()
        _check(lib().kicp_occ_level(self._h, int(level), None, 0, C.byref(total)))
        words = np.zeros(total.value, dtype=np.uint32)
        _check(lib().kicp_occ_level(self._h, int(level), _u32(words), total.value, None))
        dims = self.info()["dims"]
        return words.reshape(int(dims[2]), int(dims[1]), -1)
