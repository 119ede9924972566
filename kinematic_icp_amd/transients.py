"""Transient obstacles (kicp_transients_from_counts): the returns of one frame that end in cells the counters know as free, grouped
into transients, as pure host code.  OccupancyGrid.transients and .transients_device run the detection on the GPU and take their
argument checks from here."""
import ctypes as C

import numpy as np

from ._ffi import KICP_ERR_ARG, KICP_ERR_CAPACITY, KicpError, _check, _declare, _dp, _frame_args, _szp, _u8, _u8p, _u16, _u16p, _u32, _u32p, _u64, _u64p, lib


class TransientConfig(C.Structure):
    """kicp_transient_config: the readout's min_observations, the largest readout that is known free (0 .. 100), the returns a cell needs,
    and the least size in cells of a transient that is output and enters the plane"""
    _fields_ = [("min_observations", C.c_uint), ("free_max", C.c_uint), ("min_points", C.c_uint), ("min_size", C.c_uint)]


_ENTRIES = _declare({
    "kicp_transients_from_counts": (C.c_int, [_u16p, C.c_void_p, _dp, C.c_size_t, _dp, _dp, C.POINTER(TransientConfig), _u64p, C.c_size_t, _szp, _u32p,
                                              C.c_size_t, _u64p, _u8p, C.c_size_t]),
})

TRANSIENT_WORDS = 10


def _transient_config(min_observations, free_max, min_points, min_size):
    args = [int(min_observations), int(free_max), int(min_points), int(min_size)]
    if min(args) < 0 or max(args) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "min_observations, free_max, min_points and min_size are unsigned 32-bit integers")
    return TransientConfig(*args)


def _transient_call(call, shape, return_labels, return_stats):
    """call(rows pointer, cap, byref(n), labels pointer, cap_labels, stats pointer) -> rc, with a modest capacity first and, when more
    transients pass the filter than that, once more with the number that came back -> uint64 (T, 10), then - as asked for - uint32
    labels of `shape` and the four statistics as a tuple"""
    labels = np.empty(shape, dtype=np.uint32) if return_labels else None
    lp, lcap = (_u32(labels), labels.size) if return_labels else (None, 0)
    stats = np.zeros(4, dtype=np.uint64)
    cap, n = 64, C.c_size_t()
    rows = np.empty((cap, TRANSIENT_WORDS), dtype=np.uint64)
    rc = call(_u64(rows), cap, C.byref(n), lp, lcap, _u64(stats))
    if rc == KICP_ERR_CAPACITY and n.value > cap:  # more transients than that: their number came back
        cap = n.value
        rows = np.empty((cap, TRANSIENT_WORDS), dtype=np.uint64)
        rc = call(_u64(rows), cap, C.byref(n), lp, lcap, _u64(stats))
    _check(rc)
    out = (rows[:n.value].copy(),) + ((labels,) if return_labels else ()) + ((tuple(int(v) for v in stats),) if return_stats else ())
    return out if len(out) > 1 else out[0]


def transients_from_counts(counts, grid_config, frame, pose, sensor_xyz=(0.0, 0.0, 0.0), min_observations=1, free_max=65, min_points=1, min_size=1,
                           return_labels=False, return_stats=False, return_plane=False):
    """kicp_transients_from_counts: the transients of one frame of points in the base frame at `pose` over counters shaped (height,
    width, 2) - OccupancyGrid.counts()' layout - of a grid with `grid_config` = (cell, origin_x, origin_y, width, height, z_min, z_max,
    max_ray), OccupancyGrid's arguments.  A cell is a transient cell when at least min_points used points end in it and its readout v at
    min_observations has 0 <= v <= free_max; the cells are joined over their eight neighbours.  -> uint64 (T, 10), ascending labels, of
    the transients of at least min_size cells: label (the least cell index y * width + x), size, returns, sum of n x, sum of n y, min x,
    max x, min y, max y, and nearest = d2 * 2^32 + cell of the cell nearest the sensor's.  return_labels: also uint32 (height, width), the
    label on every transient cell - of the small transients too - and 0xFFFFFFFF elsewhere; return_stats: (points used, used points
    that end inside the grid, cells with a return, transient cells); return_plane: uint8 (height, width), 1 on the cells of the
    transients that are output.  Pure host code: needs no GPU."""
    from .grid import GridConfig  # (grid.py imports this module)
    cell, origin_x, origin_y, width, height, z_min, z_max, max_ray = grid_config
    g = GridConfig(float(cell), float(origin_x), float(origin_y), int(width), int(height), float(z_min), float(z_max), float(max_ray))
    c = np.ascontiguousarray(counts, dtype=np.uint16)
    if c.shape != (g.height, g.width, 2):
        raise KicpError(KICP_ERR_ARG, "counts must be shaped (height, width, 2): hits, misses")
    cfg = _transient_config(min_observations, free_max, min_points, min_size)
    plane = np.empty((g.height, g.width), dtype=np.uint8) if return_plane else None
    tail = (_u8(plane), plane.size) if return_plane else (None, 0)
    head = (_u16(c), C.byref(g), *_frame_args(pose, sensor_xyz, frame=frame), C.byref(cfg))
    out = _transient_call(lambda *mid: lib().kicp_transients_from_counts(*head, *mid, *tail), (g.height, g.width), return_labels, return_stats)
    if not return_plane:
        return out
    return (out if isinstance(out, tuple) else (out,)) + (plane,)
