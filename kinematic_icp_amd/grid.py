"""The 2-D occupancy grid (kicp_grid_*): the counters a mapping run draws frame by frame, their readout and map files, clearance and
Nav2-style costmaps, the fill from another grid - and, on the grid's handle, the plan (plan.py), the exploration (explore.py) and the
transient obstacles (transients.py)."""
import ctypes as C
import math
import os

import numpy as np

from ._ffi import (KICP_ERR_ARG, Handle, KicpError, _check, _declare, _dp, _frame_args, _hp, _i8, _i8p, _info, _last_window, _occupancy_2d,
                   _out_array, _rect, _szp, _u8, _u8p, _u16, _u16p, _u32, _u32p, _u64, _u64p, lib)
from .explore import GAIN_WORDS, FrontierConfig, GainConfig, _frontier_call, _frontier_config, _gain_config, _gain_views
from .transients import TransientConfig, _transient_call, _transient_config
from .plan import MAX_POTENTIAL, PlanConfig, _arc_tree_args, _arcs_args, _plan_args, _potential_out, _potential_result


class GridConfig(C.Structure):
    """kicp_grid_config: width x height cells of side `cell` from (origin_x, origin_y); points with z_min <= z < z_max (base frame) whose
    cell lies within ceil(max_ray / cell) cells of the sensor's count"""
    _fields_ = [("cell", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double), ("width", C.c_uint), ("height", C.c_uint),
                ("z_min", C.c_double), ("z_max", C.c_double), ("max_ray", C.c_double)]


class GridClearanceConfig(C.Structure):
    """kicp_grid_clearance_config: the readout's min_observations, the threshold above which a cell is a source, whether unknown cells
    are sources too, and the radius R in cells (1 .. 254)"""
    _fields_ = [("min_observations", C.c_uint), ("occupied_thresh", C.c_double), ("unknown_is_obstacle", C.c_int), ("radius_cells", C.c_int)]


class GridFillConfig(C.Structure):
    """kicp_grid_fill_config: how OccupancyGrid.fill_unknown reads its source - the readout at min_observations (>= 1) is FREE at
    0 .. free_max (<= 100), OCCUPIED from occupied_min (free_max < occupied_min <= 101; 101: never) and otherwise says nothing"""
    _fields_ = [("min_observations", C.c_uint), ("free_max", C.c_uint), ("occupied_min", C.c_uint)]


_vp, _u, _f64, _sz = C.c_void_p, C.c_uint, C.c_double, C.c_size_t
_clear, _plan, _fill = C.POINTER(GridClearanceConfig), C.POINTER(PlanConfig), C.POINTER(GridFillConfig)
_transient_tail = [_dp, _dp, C.POINTER(TransientConfig), _u64p, _sz, _szp, _u32p, _sz, _u64p]  # pose, sensor, config, rows, labels, stats

_ENTRIES = _declare({
    "kicp_grid_create": (C.c_int, [C.POINTER(GridConfig), C.c_int, _hp]),
    "kicp_grid_destroy": (None, [_vp]),
    "kicp_grid_info": (C.c_int, [_vp, C.POINTER(GridConfig), C.POINTER(C.c_int), _u64p]),
    "kicp_grid_clear": (C.c_int, [_vp]),
    "kicp_grid_integrate": (C.c_int, [_vp, _dp, _sz, _dp, _dp, _u64p]),
    "kicp_grid_integrate_device": (C.c_int, [_vp, _vp, _sz, _dp, _dp, _u64p]),
    "kicp_grid_counts": (C.c_int, [_vp, _u16p, _sz]),
    "kicp_grid_set_counts": (C.c_int, [_vp, _u16p, _sz]),
    "kicp_grid_occupancy": (C.c_int, [_vp, _u, _i8p, _sz]),
    "kicp_grid_occupancy_from_counts": (C.c_int, [_u16p, _sz, _u, _i8p]),
    "kicp_grid_save_map": (C.c_int, [_vp, C.c_char_p, _u, _f64, _f64]),
    "kicp_grid_write_map": (C.c_int, [C.c_char_p, _i8p, _u, _u, _f64, _f64, _f64, _f64, _f64]),
    "kicp_grid_clearance": (C.c_int, [_vp, _clear, _u, _u, _u, _u, _u16p, _sz]),
    "kicp_grid_costmap": (C.c_int, [_vp, _clear, _u8p, _sz, C.c_int, _u, _u, _u, _u, _u8p, _sz]),
    "kicp_grid_clearance_from_occupancy": (C.c_int, [_i8p, _u, _u, _clear, _u, _u, _u, _u, _u16p, _sz]),
    "kicp_grid_costmap_from_occupancy": (C.c_int, [_i8p, _u, _u, _clear, _u8p, _sz, C.c_int, _u, _u, _u, _u, _u8p, _sz]),
    "kicp_grid_cost_table_nav2": (C.c_int, [_f64, C.c_int, _f64, _f64, _u8p, _sz]),
    "kicp_grid_last_window": (C.c_int, [_vp, _u32p, _u32p, _u32p, _u32p]),
    "kicp_grid_fill_unknown": (C.c_int, [_vp, _vp, _fill, _u64p]),
    "kicp_grid_fill_unknown_counts": (C.c_int, [_u16p, _u16p, _sz, _fill, _u64p]),
    # the plan and the exploration on the grid's handle (plan.py and explore.py hold their host twins)
    "kicp_grid_potential_of_costmap": (C.c_int, [_vp, _u8p, _u8p, _plan, _u32p, _sz, _u32p, _sz, _u64p]),
    "kicp_grid_potential": (C.c_int, [_vp, _clear, _u8p, _sz, C.c_int, _u8p, _plan, _u32p, _sz, _u32p, _sz, _u64p]),
    "kicp_grid_has_plan": (C.c_int, [_vp]),
    "kicp_grid_score_arcs": (C.c_int, [_vp, _dp, _dp, _sz, _u, _dp, _sz, _u32p, _sz]),
    "kicp_grid_score_arc_tree": (C.c_int, [_vp, _dp, _u, _u32p, _u32p, _dp, _dp, _sz, _u32p, _sz]),
    "kicp_grid_frontiers": (C.c_int, [_vp, C.POINTER(FrontierConfig), C.c_int, _u64p, _sz, _szp, _u32p, _sz]),
    "kicp_grid_gain": (C.c_int, [_vp, C.POINTER(GainConfig), _u32p, _sz, _u32p, _sz]),
    "kicp_grid_transients": (C.c_int, [_vp, _dp, _sz] + _transient_tail),
    "kicp_grid_transients_device": (C.c_int, [_vp, _vp, _sz] + _transient_tail),
    "kicp_grid_transient_plane": (C.c_int, [_vp, _u8p, _sz]),
    "kicp_grid_use_transients": (C.c_int, [_vp, C.c_int]),
    "kicp_grid_uses_transients": (C.c_int, [_vp]),
    # the window that follows the robot (the height layer's two entries: elevation.py)
    "kicp_grid_scroll": (C.c_int, [_vp, C.c_int, C.c_int]),
    "kicp_grid_follow": (C.c_int, [_vp, _f64, _f64, _u, _u, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kicp_grid_counts_rect": (C.c_int, [_vp, _u, _u, _u, _u, _u16p, _sz]),
    "kicp_grid_set_counts_rect": (C.c_int, [_vp, _u, _u, _u, _u, _u16p, _sz]),
    "kicp_shift_plane": (C.c_int, [_vp, _vp, _u, _u, _u, C.c_int, C.c_int]),
    "kicp_follow_shift": (C.c_int, [C.c_longlong, _u, _u, _u, C.POINTER(C.c_longlong)]),
})


def shift_plane(plane, dx, dy):
    """kicp_shift_plane: `plane`, shaped (height, width) or (height, width, k) with 1, 2, 4 or 8 bytes per cell in all (a transient
    plane, counters (height, width, 2) uint16, uint64 columns), shifted by (dx, dy) -> a new array of the same shape and dtype:
    out[iy, ix] = plane[iy + dy, ix + dx] where that lies inside, 0 elsewhere.  Pure host code: needs no GPU."""
    a = np.ascontiguousarray(plane)
    if a.ndim not in (2, 3) or a.size == 0:
        raise KicpError(KICP_ERR_ARG, "the plane must be shaped (height, width) or (height, width, k), none of them 0")
    out = np.empty_like(a)
    _check(lib().kicp_shift_plane(a.ctypes.data, out.ctypes.data, a.shape[1], a.shape[0], a.itemsize * (a.shape[2] if a.ndim == 3 else 1), int(dx), int(dy)))
    return out


def follow_shift(c, size, margin, step):
    """kicp_follow_shift: the shift along one axis of `size` cells that brings cell index c into [margin, size - margin) -> int: 0 when
    it is there, else the least multiple of `step` that does (negative below the band).  Pure host code."""
    d = C.c_longlong()
    _check(lib().kicp_follow_shift(int(c), int(size), int(margin), int(step), C.byref(d)))
    return int(d.value)


def occupancy_from_counts(counts, min_observations=1):
    """kicp_grid_occupancy_from_counts: the readout of counters shaped (..., 2) = (hits, misses) on the host -> int8 of the leading shape:
    -1 below min_observations, else (100 hits + (hits + misses) / 2) / (hits + misses) in integers.  Needs no GPU."""
    c = np.ascontiguousarray(counts, dtype=np.uint16)
    if c.ndim < 1 or c.shape[-1] != 2:
        raise KicpError(KICP_ERR_ARG, "counts must be shaped (..., 2): hits, misses")
    out = np.empty(c.shape[:-1], dtype=np.int8)
    _check(lib().kicp_grid_occupancy_from_counts(_u16(c), out.size, int(min_observations), _i8(out)))
    return out


def write_map(prefix, occupancy, cell, origin_x, origin_y, occupied_thresh=0.65, free_thresh=0.25):
    """kicp_grid_write_map: `occupancy` (int8, shaped (height, width), row 0 at the origin) as <prefix>.pgm + <prefix>.yaml, the pair
    map_server and Nav2 read.  Needs no GPU."""
    occ = np.ascontiguousarray(occupancy, dtype=np.int8)
    if occ.ndim != 2:
        raise KicpError(KICP_ERR_ARG, "occupancy must be shaped (height, width)")
    _check(lib().kicp_grid_write_map(os.fsencode(prefix), _i8(occ), occ.shape[1], occ.shape[0], float(cell), float(origin_x), float(origin_y),
                                     float(occupied_thresh), float(free_thresh)))


def _clearance_config(radius_cells, min_observations, occupied_thresh, unknown_is_obstacle):
    return GridClearanceConfig(int(min_observations), float(occupied_thresh), 1 if unknown_is_obstacle else 0, int(radius_cells))


def _cost_table(table):
    t = np.ascontiguousarray(table, dtype=np.uint8)
    if t.ndim != 1:
        raise KicpError(KICP_ERR_ARG, "the cost table must be one-dimensional: table[0 .. R^2 + 1]")
    return t


def clearance_from_occupancy(occupancy, radius_cells, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, rect=None):
    """kicp_grid_clearance_from_occupancy: the squared distance in cells from every cell of `rect` = (x0, y0, w, h) (None: the full grid)
    to the nearest source within radius_cells of it, radius_cells^2 + 1 where there is none, over a readout shaped (height, width) ->
    uint16 (h, w).  Pure host code: needs no GPU."""
    occ = _occupancy_2d(occupancy)
    x0, y0, w, h = _rect(rect, occ.shape[1], occ.shape[0])
    cfg = _clearance_config(radius_cells, min_observations, occupied_thresh, unknown_is_obstacle)
    out = np.empty((h, w), dtype=np.uint16)
    _check(lib().kicp_grid_clearance_from_occupancy(_i8(occ), occ.shape[1], occ.shape[0], C.byref(cfg), x0, y0, w, h, _u16(out), out.size))
    return out


def costmap_from_occupancy(occupancy, table, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=False, rect=None):
    """kicp_grid_costmap_from_occupancy: Nav2's costs (254 lethal, 253 inscribed, 255 no information, 0 free) of the cells of `rect` from
    `table`[clearance] (length R^2 + 2, which gives R) over a readout shaped (height, width) -> uint8 (h, w).  Pure host code."""
    occ, t = _occupancy_2d(occupancy), _cost_table(table)
    x0, y0, w, h = _rect(rect, occ.shape[1], occ.shape[0])
    cfg = _clearance_config(_table_radius(t), min_observations, occupied_thresh, unknown_is_obstacle)
    out = np.empty((h, w), dtype=np.uint8)
    _check(lib().kicp_grid_costmap_from_occupancy(_i8(occ), occ.shape[1], occ.shape[0], C.byref(cfg), _u8(t), t.size, 1 if inflate_unknown else 0,
                                                  x0, y0, w, h, _u8(out), out.size))
    return out


def _table_radius(table):
    """R of a table of R^2 + 2 entries (any other length: KICP_ERR_ARG)"""
    r = math.isqrt(max(int(table.size) - 2, 0))
    if r * r + 2 != table.size:
        raise KicpError(KICP_ERR_ARG, "the cost table must have R^2 + 2 entries, table[0 .. R^2 + 1]")
    return r


def nav2_cost_table(cell, radius_cells, inscribed_radius, cost_scaling_factor):
    """kicp_grid_cost_table_nav2: the table of Nav2's inflation layer for a radius of radius_cells cells of `cell` metres -> uint8
    [radius_cells^2 + 2]: 254 at 0, 253 up to inscribed_radius, 252 exp(-cost_scaling_factor (d - inscribed_radius)) beyond, 0 for far"""
    r = int(radius_cells)
    out = np.empty(r * r + 2 if 1 <= r <= 254 else 2, dtype=np.uint8)
    _check(lib().kicp_grid_cost_table_nav2(float(cell), r, float(inscribed_radius), float(cost_scaling_factor), _u8(out), out.size))
    return out


def fill_unknown_counts(dst_counts, src_counts, min_observations=1, free_max=25, occupied_min=101, return_counts=False):
    """kicp_grid_fill_unknown_counts: OccupancyGrid.fill_unknown as pure host code over counters in counts()' layout - uint16 (..., 2),
    the same shape - -> the destination's counters after the fill, a new array (the arguments are not changed); return_counts adds
    the seven counts.  Needs no GPU."""
    d, s = np.array(dst_counts, dtype=np.uint16, order="C"), np.ascontiguousarray(src_counts, dtype=np.uint16)
    if d.shape != s.shape or d.size % 2:
        raise KicpError(KICP_ERR_ARG, "the two arrays must have one shape and hold (hits, misses) pairs")
    cfg, counts = GridFillConfig(int(min_observations), int(free_max), int(occupied_min)), np.zeros(7, dtype=np.uint64)
    _check(lib().kicp_grid_fill_unknown_counts(_u16(d), _u16(s), d.size // 2, C.byref(cfg), _u64(counts) if return_counts else None))
    return (d, tuple(int(v) for v in counts)) if return_counts else d


class OccupancyGrid(Handle):
    """kicp_grid: a world-aligned 2-D grid of (hits, misses) counters a mapping run draws frame by frame - every used point's cell is
    hit, the cells its ray from the sensor crosses are missed, once per cell per frame (include/kicp.h states the exact semantics).
    It owns its device memory; the counters stay in HBM until they are asked for."""

    _destroy = "kicp_grid_destroy"

    def __init__(self, cell, origin_x, origin_y, width, height, z_min, z_max, max_ray, device=0):
        cfg = GridConfig(float(cell), float(origin_x), float(origin_y), int(width), int(height), float(z_min), float(z_max), float(max_ray))
        self._create("kicp_grid_create", C.byref(cfg), int(device))
        self.device, self.width, self.height = device, int(width), int(height)
        self._last = np.zeros(4, dtype=np.uint64)

    def info(self):
        """-> dict: the configuration's fields, reach (cells) and frames (integrated since creation or clear)"""
        return _info("kicp_grid_info", self._h, GridConfig(), reach=C.c_int(), frames=C.c_ulonglong())

    def clear(self):
        _check(lib().kicp_grid_clear(self._h))

    def integrate(self, frame, pose, sensor_xyz=(0.0, 0.0, 0.0)):
        """kicp_grid_integrate: one frame of points in the base frame (host memory) at `pose`, the sensor at `sensor_xyz` in the base frame
        -> (points used, points skipped, cells HIT, cells MISS)"""
        _check(lib().kicp_grid_integrate(self._h, *_frame_args(pose, sensor_xyz, frame=frame), _u64(self._last)))
        return self.last_frame()

    def integrate_device(self, device_frame, pose, sensor_xyz=(0.0, 0.0, 0.0), n=None):
        """kicp_grid_integrate_device: the same for a DeviceFrame (or anything with .ptr and .n) already in HBM"""
        _check(lib().kicp_grid_integrate_device(self._h, *_frame_args(pose, sensor_xyz, device_frame=device_frame, n=n), _u64(self._last)))
        return self.last_frame()

    def last_frame(self):
        """(points used, points skipped, cells HIT, cells MISS) of the last integrated frame"""
        return tuple(int(v) for v in self._last)

    def counts(self):
        """-> uint16 (height, width, 2): hits, misses"""
        out = np.empty((self.height, self.width, 2), dtype=np.uint16)
        _check(lib().kicp_grid_counts(self._h, _u16(out), self.width * self.height))
        return out

    def set_counts(self, counts):
        c = np.ascontiguousarray(counts, dtype=np.uint16)
        if c.size % 2:
            raise KicpError(KICP_ERR_ARG, "counts must hold (hits, misses) pairs")
        _check(lib().kicp_grid_set_counts(self._h, _u16(c), c.size // 2))

    def counts_rect(self, rect):
        """kicp_grid_counts_rect: the counters of `rect` = (x0, y0, w, h), inside the grid -> uint16 (h, w, 2)"""
        x0, y0, w, h = _rect(rect, self.width, self.height)
        out = np.empty((h, w, 2), dtype=np.uint16)
        _check(lib().kicp_grid_counts_rect(self._h, x0, y0, w, h, _u16(out), out.size // 2))
        return out

    def set_counts_rect(self, rect, counts):
        """kicp_grid_set_counts_rect: writes `counts`, uint16 (h, w, 2), over the cells of `rect` = (x0, y0, w, h); every other cell and
        the plan stay"""
        x0, y0, w, h = _rect(rect, self.width, self.height)
        c = np.ascontiguousarray(counts, dtype=np.uint16)
        if c.size % 2:
            raise KicpError(KICP_ERR_ARG, "counts must hold (hits, misses) pairs")
        _check(lib().kicp_grid_set_counts_rect(self._h, x0, y0, w, h, _u16(c), c.size // 2))

    def scroll(self, dx, dy):
        """kicp_grid_scroll: on the GPU, the window moves by (dx, dy) cells: cell (ix, iy) afterwards holds what (ix + dx, iy + dy) held,
        cells that enter are unknown, the transient plane moves along, the origin becomes origin + d * cell, the last window is
        translated and the plan is invalidated.  (0, 0) changes nothing."""
        _check(lib().kicp_grid_scroll(self._h, int(dx), int(dy)))

    def follow(self, x, y, margin, step):
        """kicp_grid_follow: scrolls, in multiples of `step` cells per axis, so that the cell of the world position (x, y) lies at least
        `margin` cells from every edge -> the (dx, dy) applied; (0, 0), the common case, costs no launch"""
        dx, dy = C.c_int(), C.c_int()
        _check(lib().kicp_grid_follow(self._h, float(x), float(y), int(margin), int(step), C.byref(dx), C.byref(dy)))
        return int(dx.value), int(dy.value)

    def fill_unknown(self, src, min_observations=1, free_max=25, occupied_min=101, return_counts=False):
        """kicp_grid_fill_unknown: on the GPU, the unknown cells of this grid - both counters 0 - become traversable (0, 1) where `src`,
        an OccupancyGrid of the same geometry, reads 0 .. free_max at min_observations, and obstacles (1, 0) where it reads occupied_min
        or more (101: never); every other counter keeps its bits, `src` is not changed, and the plan of this grid is invalidated.
        return_counts -> (kept obstacle, kept traversable, filled free, filled occupied, left unknown, traversable over a source
        OCCUPIED, obstacle over a source FREE)"""
        cfg, counts = GridFillConfig(int(min_observations), int(free_max), int(occupied_min)), np.zeros(7, dtype=np.uint64)
        _check(lib().kicp_grid_fill_unknown(self._h, src._h if src is not None else None, C.byref(cfg), _u64(counts) if return_counts else None))
        return tuple(int(v) for v in counts) if return_counts else None

    def occupancy(self, min_observations=1):
        """kicp_grid_occupancy: the readout on the GPU -> int8 (height, width): -1 unknown, else 0 .. 100 - a nav_msgs/OccupancyGrid's data"""
        out = np.empty((self.height, self.width), dtype=np.int8)
        _check(lib().kicp_grid_occupancy(self._h, int(min_observations), _i8(out), out.size))
        return out

    def clearance(self, radius_cells, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, rect=None):
        """kicp_grid_clearance: on the GPU, the squared distance in cells from every cell of `rect` = (x0, y0, w, h) (None: the full grid)
        to the nearest source within radius_cells of it - inside the rectangle or not - radius_cells^2 + 1 where there is none
        -> uint16 (h, w)"""
        x0, y0, w, h = _rect(rect, self.width, self.height)
        cfg = _clearance_config(radius_cells, min_observations, occupied_thresh, unknown_is_obstacle)
        out = np.empty((h, w), dtype=np.uint16)
        _check(lib().kicp_grid_clearance(self._h, C.byref(cfg), x0, y0, w, h, _u16(out), out.size))
        return out

    def costmap(self, table, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=False, rect=None):
        """kicp_grid_costmap: on the GPU, Nav2's costs of the cells of `rect` from `table`[clearance] (nav2_cost_table builds one; its
        length R^2 + 2 gives R) -> uint8 (h, w): a nav2_msgs/Costmap's data"""
        t = _cost_table(table)
        x0, y0, w, h = _rect(rect, self.width, self.height)
        cfg = _clearance_config(_table_radius(t), min_observations, occupied_thresh, unknown_is_obstacle)
        out = np.empty((h, w), dtype=np.uint8)
        _check(lib().kicp_grid_costmap(self._h, C.byref(cfg), _u8(t), t.size, 1 if inflate_unknown else 0, x0, y0, w, h, _u8(out), out.size))
        return out

    def potential_of_costmap(self, costmap, weight, goals, max_potential=MAX_POTENTIAL, return_stats=False, out=None):
        """kicp_grid_potential_of_costmap: on the GPU, the cost-to-go field of potential_from_costmap over `costmap` (uint8, the grid's
        (height, width)) -> uint32 (height, width).  return_stats: also (goals used, cells below max_potential, cells at it, relaxation
        rounds - the last depends on the implementation); out: as potential_from_costmap's."""
        cm, wt, g, cfg = _plan_args(costmap, weight, goals, max_potential)
        if cm.shape != (self.height, self.width):
            raise KicpError(KICP_ERR_ARG, "the costmap must have the grid's shape (height, width)")
        out, stats = _potential_out(out, cm.shape), np.zeros(4, dtype=np.uint64)
        _check(lib().kicp_grid_potential_of_costmap(self._h, _u8(cm), _u8(wt), C.byref(cfg), _u32(g), len(g), _u32(out), out.size, _u64(stats)))
        return _potential_result(out, stats, return_stats)

    def potential(self, table, weight, goals, max_potential=MAX_POTENTIAL, min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=False,
                  return_stats=False, out=None):
        """kicp_grid_potential: on the GPU, the full grid's costmap (the arguments and bytes of costmap()) and the cost-to-go field over
        it from `goals` = [(x, y), ...] - the costmap never leaves HBM -> uint32 (height, width); return_stats and out as
        potential_of_costmap's"""
        t = _cost_table(table)
        cfg = _clearance_config(_table_radius(t), min_observations, occupied_thresh, unknown_is_obstacle)
        _, wt, g, plan = _plan_args(np.zeros((1, 1), dtype=np.uint8), weight, goals, max_potential)
        out, stats = _potential_out(out, (self.height, self.width)), np.zeros(4, dtype=np.uint64)
        _check(lib().kicp_grid_potential(self._h, C.byref(cfg), _u8(t), t.size, 1 if inflate_unknown else 0, _u8(wt), C.byref(plan), _u32(g), len(g),
                                         _u32(out), out.size, _u64(stats)))
        return _potential_result(out, stats, return_stats)

    def has_plan(self):
        """kicp_grid_has_plan: does the handle hold the plan of a potential call that succeeded?"""
        return bool(lib().kicp_grid_has_plan(self._h))

    def score_arcs(self, start, arcs, n_steps, footprint, out=None):
        """kicp_grid_score_arcs: on the GPU, score_arcs_from_plan's result on the plan the last potential() or potential_of_costmap()
        left in the handle (KICP_ERR_ARG when there is none) -> uint32 (K, 4); the plan never leaves HBM.  out: as
        score_arcs_from_plan's."""
        s, a, f, n_steps = _arcs_args(start, arcs, n_steps, footprint)
        out = _out_array(out, (len(a), 4), np.uint32, "(K, 4)")
        _check(lib().kicp_grid_score_arcs(self._h, C.cast(s.ctypes.data, _dp), C.cast(a.ctypes.data, _dp), len(a), n_steps, C.cast(f.ctypes.data, _dp), len(f),
                                          _u32(out), out.size))
        return out

    def score_arc_tree(self, start, branch, steps, primitives, footprint, out=None):
        """kicp_grid_score_arc_tree: on the GPU, score_arc_tree_from_plan's result on the plan the last potential() or
        potential_of_costmap() left in the handle (KICP_ERR_ARG when there is none) -> uint32 (N, 4), one launch per level; the plan
        never leaves HBM.  out: as score_arc_tree_from_plan's."""
        s, b, st, p, f, n_nodes = _arc_tree_args(start, branch, steps, primitives, footprint)
        out = _out_array(out, (n_nodes, 4), np.uint32, "(N, 4) = (%d, 4)" % n_nodes)
        _check(lib().kicp_grid_score_arc_tree(self._h, C.cast(s.ctypes.data, _dp), b.size, _u32(b), _u32(st), C.cast(p.ctypes.data, _dp),
                                              C.cast(f.ctypes.data, _dp), len(f), _u32(out), out.size))
        return out

    def frontiers(self, min_observations=1, occupied_thresh=0.65, min_size=1, use_plan=False, return_labels=False):
        """kicp_grid_frontiers: on the GPU, frontiers_from_occupancy's result on the counters where they are -> uint64 (F, 10), and uint32
        (height, width) labels with return_labels.  use_plan: best_potential and best_cell come from the plan the last potential() or
        potential_of_costmap() left in the handle (KICP_ERR_ARG when there is none) - with the robot's cell as that call's one goal,
        the cost of driving to each frontier and the cell to drive to.  The plan is a snapshot, the frontiers are the current counters';
        neither is changed."""
        cfg = _frontier_config(min_observations, occupied_thresh, min_size)
        return _frontier_call(lambda *tail: lib().kicp_grid_frontiers(self._h, C.byref(cfg), 1 if use_plan else 0, *tail), (self.height, self.width),
                              return_labels)

    def gain(self, views, range_cells, min_observations=1, occupied_thresh=0.65):
        """kicp_grid_gain: on the GPU, gain_from_occupancy's result on the counters where they are -> uint32 (N, 4): per viewpoint (a cell
        index, such as frontiers(use_plan=True)[:, 9], or (x, y)) the distinct unknown cells a sensor of range_cells' range would see, the
        rays blocked, the rays that left the grid and the class of the viewpoint's cell.  Neither the counters nor the plan are changed."""
        cfg = _gain_config(range_cells, min_observations, occupied_thresh)
        v = _gain_views(views, self.width, self.height)
        out = np.empty((len(v), GAIN_WORDS), dtype=np.uint32)
        _check(lib().kicp_grid_gain(self._h, C.byref(cfg), _u32(v), len(v), _u32(out), out.size))
        return out

    def transients(self, frame, pose, sensor_xyz=(0.0, 0.0, 0.0), min_observations=1, free_max=65, min_points=1, min_size=1, return_labels=False,
                   return_stats=False):
        """kicp_grid_transients: on the GPU, transients_from_counts' result for one frame of points in the base frame (host memory) at
        `pose` on the counters where they are -> uint64 (T, 10), then uint32 (height, width) labels with return_labels and (points used,
        used points that end inside the grid, cells with a return, transient cells) with return_stats.  Call it before integrate() of
        the same frame.  The counters, the frame count, the last window and the plan are not changed; the handle's transient plane is
        replaced by the cells of the transients that are output."""
        cfg = _transient_config(min_observations, free_max, min_points, min_size)
        head = (self._h, *_frame_args(pose, sensor_xyz, frame=frame), C.byref(cfg))
        return _transient_call(lambda *tail: lib().kicp_grid_transients(*head, *tail), (self.height, self.width), return_labels, return_stats)

    def transients_device(self, device_frame, pose, sensor_xyz=(0.0, 0.0, 0.0), n=None, min_observations=1, free_max=65, min_points=1, min_size=1,
                          return_labels=False, return_stats=False):
        """kicp_grid_transients_device: the same for a DeviceFrame (or anything with .ptr and .n) already in HBM"""
        cfg = _transient_config(min_observations, free_max, min_points, min_size)
        head = (self._h, *_frame_args(pose, sensor_xyz, device_frame=device_frame, n=n), C.byref(cfg))
        return _transient_call(lambda *tail: lib().kicp_grid_transients_device(*head, *tail), (self.height, self.width), return_labels, return_stats)

    def transient_plane(self):
        """kicp_grid_transient_plane: -> uint8 (height, width), 1 on the cells of the last transients() call's transients that passed
        min_size; all 0 before the first call, after clear() and after a call that found none"""
        out = np.empty((self.height, self.width), dtype=np.uint8)
        _check(lib().kicp_grid_transient_plane(self._h, _u8(out), out.size))
        return out

    def use_transients(self, on=True):
        """kicp_grid_use_transients: while on, the transient plane's cells are sources in clearance(), costmap() and potential() whatever
        their counters say; everything else ignores the plane.  Off at creation; clear() does not change it."""
        _check(lib().kicp_grid_use_transients(self._h, 1 if on else 0))

    def uses_transients(self):
        """kicp_grid_uses_transients: is the switch on?"""
        return bool(lib().kicp_grid_uses_transients(self._h))

    def last_window(self):
        """kicp_grid_last_window: (x0, y0, w, h) of the last integrated frame's window clipped to the grid; w = h = 0 when it lies
        outside and before any frame.  Grown by R and clipped it is all a costmap has to refresh after that frame."""
        return _last_window("kicp_grid_last_window", self._h)

    def save_map(self, prefix, min_observations=1, occupied_thresh=0.65, free_thresh=0.25):
        """kicp_grid_save_map: <prefix>.pgm + <prefix>.yaml of the readout"""
        _check(lib().kicp_grid_save_map(self._h, os.fsencode(prefix), int(min_observations), float(occupied_thresh), float(free_thresh)))
