"""Exploration over an occupancy readout as pure host code (kicp_frontiers_from_occupancy, kicp_gain_from_occupancy): frontiers and the
unknown cells a viewpoint would reveal.  OccupancyGrid.frontiers and .gain run them on the GPU and take their argument checks from
here."""
import ctypes as C

import numpy as np

from ._ffi import KICP_ERR_ARG, KICP_ERR_CAPACITY, KicpError, _check, _declare, _i8, _i8p, _occupancy_2d, _szp, _u32, _u32p, _u64, _u64p, lib


class FrontierConfig(C.Structure):
    """kicp_frontier_config: the readout's min_observations, the threshold above which a cell is occupied, and the least size in cells
    of a frontier that is output"""
    _fields_ = [("min_observations", C.c_uint), ("occupied_thresh", C.c_double), ("min_size", C.c_uint)]


class GainConfig(C.Structure):
    """kicp_gain_config: the readout's min_observations, the threshold above which a cell is occupied, and the sensor's range R in cells
    (1 .. 361)"""
    _fields_ = [("min_observations", C.c_uint), ("occupied_thresh", C.c_double), ("range_cells", C.c_uint)]


_ENTRIES = _declare({
    "kicp_frontiers_from_occupancy": (C.c_int, [_i8p, C.c_uint, C.c_uint, C.POINTER(FrontierConfig), _u32p, _u64p, C.c_size_t, _szp, _u32p, C.c_size_t]),
    "kicp_gain_from_occupancy": (C.c_int, [_i8p, C.c_uint, C.c_uint, C.POINTER(GainConfig), _u32p, C.c_size_t, _u32p, C.c_size_t]),
})

FRONTIER_WORDS = 10


def _frontier_config(min_observations, occupied_thresh, min_size):
    args = [int(min_observations), int(min_size)]
    if min(args) < 0 or max(args) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "min_observations and min_size are unsigned 32-bit integers, at least 1")
    return FrontierConfig(args[0], float(occupied_thresh), args[1])


def _frontier_call(call, shape, return_labels):
    """call(rows pointer, cap, byref(n), labels pointer, cap_labels) -> rc, with a modest capacity first and, when more frontiers pass the
    filter than that, once more with the number that came back -> uint64 (F, 10), or that and uint32 labels of `shape`"""
    labels = np.empty(shape, dtype=np.uint32) if return_labels else None
    lp, lcap = (_u32(labels), labels.size) if return_labels else (None, 0)
    cap, n = 256, C.c_size_t()
    rows = np.empty((cap, FRONTIER_WORDS), dtype=np.uint64)
    rc = call(_u64(rows), cap, C.byref(n), lp, lcap)
    if rc == KICP_ERR_CAPACITY and n.value > cap:  # more frontiers than that: their number came back
        cap = n.value
        rows = np.empty((cap, FRONTIER_WORDS), dtype=np.uint64)
        rc = call(_u64(rows), cap, C.byref(n), lp, lcap)
    _check(rc)
    rows = rows[:n.value].copy()
    return (rows, labels) if return_labels else rows


def frontiers_from_occupancy(occupancy, min_observations=1, occupied_thresh=0.65, min_size=1, potential=None, return_labels=False):
    """kicp_frontiers_from_occupancy: the exploration frontiers of a readout shaped (height, width) - the clear cells with an unknown edge
    neighbour, joined over their eight neighbours - of at least min_size cells, in ascending label order -> uint64 (F, 10): label (the
    least cell index y * width + x), size, sum of x, sum of y, min x, max x, min y, max y, best_potential (the least of `potential`,
    uint32 (height, width), over the cells; 0xFFFFFFFF without one) and best_cell (the least index that attains it).  return_labels:
    also uint32 (height, width), the label on every frontier cell - of the small frontiers too - and 0xFFFFFFFF elsewhere.  Pure host
    code: needs no GPU."""
    occ = _occupancy_2d(occupancy)
    cfg = _frontier_config(min_observations, occupied_thresh, min_size)
    pot = None
    if potential is not None:
        pot = np.ascontiguousarray(potential, dtype=np.uint32)
        if pot.shape != occ.shape:
            raise KicpError(KICP_ERR_ARG, "the potential must have the occupancy's shape")
    head = (_i8(occ), occ.shape[1], occ.shape[0], C.byref(cfg), None if pot is None else _u32(pot))
    return _frontier_call(lambda *tail: lib().kicp_frontiers_from_occupancy(*head, *tail), occ.shape, return_labels)


GAIN_WORDS = 4


def _gain_config(range_cells, min_observations, occupied_thresh):
    args = [int(min_observations), int(range_cells)]
    if min(args) < 0 or max(args) > 0xFFFFFFFF:
        raise KicpError(KICP_ERR_ARG, "min_observations and range_cells are unsigned 32-bit integers, at least 1")
    return GainConfig(args[0], float(occupied_thresh), args[1])


def _gain_views(views, width, height):
    """viewpoints as cell indices y * width + x (any shape but (N, 2): flattened) or as an (N, 2) array of (x, y) -> uint32 (N,)"""
    v = np.asarray(views)
    if v.size and v.dtype.kind not in "iu":
        raise KicpError(KICP_ERR_ARG, "viewpoints are integers: cell indices, or an (N, 2) array of (x, y)")
    v = v.astype(np.int64)
    if v.ndim == 2 and v.shape[1] == 2:
        if v.size and not ((v >= 0).all() and (v[:, 0] < width).all() and (v[:, 1] < height).all()):
            bad = int(np.flatnonzero((v < 0).any(axis=1) | (v[:, 0] >= width) | (v[:, 1] >= height))[0])
            raise KicpError(KICP_ERR_ARG, "viewpoint %d is (%d, %d), outside the grid of %d x %d cells" % (bad, v[bad, 0], v[bad, 1], width, height))
        v = v[:, 1] * width + v[:, 0]
    v = v.reshape(-1)
    if v.size and (v.min() < 0 or v.max() > 0xFFFFFFFF):
        raise KicpError(KICP_ERR_ARG, "viewpoints are cell indices, unsigned 32-bit integers")
    return np.ascontiguousarray(v, dtype=np.uint32)


def gain_from_occupancy(occupancy, views, range_cells, min_observations=1, occupied_thresh=0.65):
    """kicp_gain_from_occupancy: what a sensor of range_cells' range (1 .. 361) would see from each viewpoint of a readout shaped
    (height, width): from a clear viewpoint 8 R rays are walked to the cells at Chebyshev distance R, cut to the disc of radius R; a ray
    ends where it leaves the grid or at an occupied cell and passes through unknown cells, which it thereby sees (include/kicp.h states
    the walk).  views: cell indices y * width + x - word 9 of a frontier's row - or an (N, 2) array of (x, y) -> uint32 (N, 4): the
    distinct unknown cells seen, the rays blocked, the rays that left the grid, and the class of the viewpoint's own cell (0 clear,
    1 unknown, 2 occupied: then the other three are 0).  Pure host code: needs no GPU."""
    occ = _occupancy_2d(occupancy)
    cfg = _gain_config(range_cells, min_observations, occupied_thresh)
    v = _gain_views(views, occ.shape[1], occ.shape[0])
    out = np.empty((len(v), GAIN_WORDS), dtype=np.uint32)
    _check(lib().kicp_gain_from_occupancy(_i8(occ), occ.shape[1], occ.shape[0], C.byref(cfg), _u32(v), len(v), _u32(out), out.size))
    return out
