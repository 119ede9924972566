"""Height columns per grid cell (kicp_elev_*): the layer that keeps them on the GPU, carving along a frame's rays, and traversability -
plain, with a slope limit, with the class ROUGH - read off them on the GPU or, by the *_from_columns functions, on the host.  A grid
the classes are written into is touched through its handle only."""
import ctypes as C

import numpy as np

from ._ffi import (KICP_ERR_ARG, Handle, KicpError, _check, _declare, _dp, _frame_args, _hp, _i8, _i8p, _info, _last_window, _rect, _u8, _u8p, _u32p,
                   _u64, _u64p, _i64p, lib)


class ElevationConfig(C.Structure):
    """kicp_elev_config: the grid's geometry - width x height cells of side `cell` from (origin_x, origin_y), max_ray - and a vertical
    one: bit b of a cell's 64-bit column is the world heights [z_origin + b slab, z_origin + (b + 1) slab)"""
    _fields_ = [("cell", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double), ("width", C.c_uint), ("height", C.c_uint),
                ("z_origin", C.c_double), ("slab", C.c_double), ("max_ray", C.c_double)]


class ElevationTraversabilityConfig(C.Structure):
    """kicp_elev_traversability_config: the highest step the robot takes (0 .. 62) and its height (step_slabs < robot_slabs <= 64), in slabs"""
    _fields_ = [("step_slabs", C.c_uint), ("robot_slabs", C.c_uint)]


class ElevationCarveConfig(C.Structure):
    """kicp_elev_carve_config: the last margin_steps steps of every ray before its endpoint cell are not carved, each step's span of slabs
    is widened by widen_slabs (0 .. 64) on both sides, and with keep_ground (0 or 1) the lowest set bit of a column is never cleared"""
    _fields_ = [("margin_steps", C.c_uint), ("widen_slabs", C.c_uint), ("keep_ground", C.c_uint)]


class ElevationSlopeConfig(C.Structure):
    """kicp_elev_slope_config: the plane fit of the slope limit - a window of radius_cells (1 .. 8) around each cell, of which the cells
    count whose ground differs from the cell's by at most gate_slabs (0 .. 63); at least min_cells (3 .. 289) of them; the limit is
    rise_slabs (0 .. 65535) slabs of height per run_cells (1 .. 65535) cells of distance"""
    _fields_ = [("radius_cells", C.c_uint), ("gate_slabs", C.c_uint), ("min_cells", C.c_uint), ("rise_slabs", C.c_uint), ("run_cells", C.c_uint)]


class ElevationRoughConfig(C.Structure):
    """kicp_elev_rough_config: the class ROUGH of the slope limit's plane fit - a cell with a fit is ROUGH when the mean squared residual
    of its fit set to the fitted plane exceeds num (0 .. 65535) / den (1 .. 65535) slabs^2"""
    _fields_ = [("num", C.c_uint), ("den", C.c_uint)]


_vp, _u, _sz = C.c_void_p, C.c_uint, C.c_size_t
_cfg, _trav, _carve = C.POINTER(ElevationConfig), C.POINTER(ElevationTraversabilityConfig), C.POINTER(ElevationCarveConfig)
_slope, _rough = C.POINTER(ElevationSlopeConfig), C.POINTER(ElevationRoughConfig)
_rect_out = [_u, _u, _u, _u, _i8p, _u8p]  # x0, y0, w, h, the classes, the ground bytes; then the fit (where there is one), the counts, the capacity

_ENTRIES = _declare({
    "kicp_elev_create": (C.c_int, [_cfg, C.c_int, _hp]),
    "kicp_elev_destroy": (None, [_vp]),
    "kicp_elev_info": (C.c_int, [_vp, _cfg, C.POINTER(C.c_int), _u64p]),
    "kicp_elev_clear": (C.c_int, [_vp]),
    "kicp_elev_integrate": (C.c_int, [_vp, _dp, _sz, _dp, _dp, _u64p]),
    "kicp_elev_integrate_device": (C.c_int, [_vp, _vp, _sz, _dp, _dp, _u64p]),
    "kicp_elev_update": (C.c_int, [_vp, _dp, _sz, _dp, _dp, _carve, _u64p]),
    "kicp_elev_update_device": (C.c_int, [_vp, _vp, _sz, _dp, _dp, _carve, _u64p]),
    "kicp_elev_update_columns": (C.c_int, [_cfg, _u64p, _sz, _dp, _sz, _dp, _dp, _carve, _u64p]),
    "kicp_elev_columns": (C.c_int, [_vp, _u64p, _sz]),
    "kicp_elev_set_columns": (C.c_int, [_vp, _u64p, _sz]),
    "kicp_elev_last_window": (C.c_int, [_vp, _u32p, _u32p, _u32p, _u32p]),
    "kicp_elev_scroll": (C.c_int, [_vp, C.c_int, C.c_int]),
    "kicp_elev_follow": (C.c_int, [_vp, C.c_double, C.c_double, C.c_uint, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kicp_elev_traversability": (C.c_int, [_vp, _trav] + _rect_out + [_u64p, _sz]),
    "kicp_elev_traversability_from_columns": (C.c_int, [_u64p, _u, _u, _trav] + _rect_out + [_u64p, _sz]),
    "kicp_elev_to_grid": (C.c_int, [_vp, _trav, _vp]),
    "kicp_elev_traversability_slope": (C.c_int, [_vp, _trav, _slope] + _rect_out + [_i64p, _u64p, _sz]),
    "kicp_elev_traversability_slope_from_columns": (C.c_int, [_u64p, _u, _u, _trav, _slope] + _rect_out + [_i64p, _u64p, _sz]),
    "kicp_elev_to_grid_slope": (C.c_int, [_vp, _trav, _slope, _vp]),
    "kicp_elev_slope_limit": (C.c_int, [_cfg, C.c_double, _u32p, _u32p]),
    "kicp_elev_traversability_rough": (C.c_int, [_vp, _trav, _slope, _rough] + _rect_out + [_i64p, _u64p, _sz]),
    "kicp_elev_traversability_rough_from_columns": (C.c_int, [_u64p, _u, _u, _trav, _slope, _rough] + _rect_out + [_i64p, _u64p, _sz]),
    "kicp_elev_to_grid_rough": (C.c_int, [_vp, _trav, _slope, _rough, _vp]),
    "kicp_elev_rough_limit": (C.c_int, [_cfg, C.c_double, _u32p, _u32p]),
})


def _struct(cls, value):
    """a ctypes struct of integers: an instance of cls, or its fields as a tuple or a dict"""
    if isinstance(value, cls):
        return value
    if isinstance(value, dict):
        value = [value[name] for name, _ in cls._fields_]
    return cls(*[int(v) for v in value])


def _traversability_call(call, w, h, return_ground, return_fit, return_counts, fit_values, count_words):
    """what the traversability entries share: the outputs, the call, and what is returned - the classes alone, or a tuple with the
    ground bytes, the fit and / or the counts behind them.  fit_values = 0: the entry has no fit argument; 3: the fit is int64 (h, w, 3)
    - D, Da, Db - and the counts are five; 5: with ROUGH (h, w, 5) - D, Da, Db, Q, n - and six"""
    out = np.empty((h, w), dtype=np.int8)
    ground = np.empty((h, w), dtype=np.uint8) if return_ground else None
    fit = np.empty((h, w, fit_values), dtype=np.int64) if return_fit else None
    counts = np.zeros(count_words, dtype=np.uint64)
    fit_arg = [fit.ctypes.data_as(_i64p) if return_fit else None] if fit_values else []
    _check(call(_i8(out), _u8(ground) if return_ground else None, *fit_arg, _u64(counts) if return_counts else None, out.size))
    if not (return_ground or return_fit or return_counts):
        return out
    return (out,) + ((ground,) if return_ground else ()) + ((fit,) if return_fit else ()) + ((tuple(int(v) for v in counts),) if return_counts else ())


def _elev_classes(step_slabs, robot_slabs, *fit):
    """a classification - plain, with a slope config, or with a slope and a rough config (each a struct, a tuple or a dict) -> the suffix
    of its entries' names, its configs by reference, fit_values and count_words (_traversability_call)"""
    cfgs = [ElevationTraversabilityConfig(int(step_slabs), int(robot_slabs))]
    cfgs += [_struct(cls, v) for cls, v in zip((ElevationSlopeConfig, ElevationRoughConfig), fit)]
    return ("", "_slope", "_rough")[len(fit)], [C.byref(v) for v in cfgs], (0, 3, 5)[len(fit)], 4 + len(fit)


def _traversability_from_columns(columns, rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, *fit):
    """what the three *_from_columns functions share"""
    c = np.ascontiguousarray(columns, dtype=np.uint64)
    if c.ndim != 2 or c.size == 0:
        raise KicpError(KICP_ERR_ARG, "columns must be shaped (height, width), both at least 1")
    x0, y0, w, h = _rect(rect, c.shape[1], c.shape[0])
    suffix, cfgs, fit_values, count_words = _elev_classes(step_slabs, robot_slabs, *fit)
    entry = getattr(lib(), "kicp_elev_traversability" + suffix + "_from_columns")
    return _traversability_call(lambda *outs: entry(_u64(c), c.shape[1], c.shape[0], *cfgs, x0, y0, w, h, *outs), w, h, return_ground, return_fit,
                                return_counts, fit_values, count_words)


def traversability_from_columns(columns, step_slabs, robot_slabs, rect=None, return_ground=False, return_counts=False):
    """kicp_elev_traversability_from_columns: the classes of the cells of `rect` = (x0, y0, w, h) (None: the full layer) from columns
    shaped (height, width), uint64 -> int8 (h, w): -1 unknown, 0 traversable, 100 obstacle (BODY: something between step_slabs and
    robot_slabs over the cell's ground; STEP: an 8-neighbour's ground more than step_slabs below).  return_ground adds uint8 (h, w), the
    ground's slab, 255 unknown; return_counts adds (unknown, traversable, BODY, STEP only).  Pure host code: needs no GPU."""
    return _traversability_from_columns(columns, rect, return_ground, False, return_counts, step_slabs, robot_slabs)


def traversability_slope_from_columns(columns, step_slabs, robot_slabs, slope, rect=None, return_ground=False, return_fit=False, return_counts=False):
    """kicp_elev_traversability_slope_from_columns: traversability_from_columns with the slope limit - a cell is also an obstacle when a
    least-squares plane through the known grounds of its window (include/kicp.h states the fit) is steeper than slope.rise_slabs slabs
    per slope.run_cells cells.  slope: an ElevationSlopeConfig, or its five fields as a tuple or a dict.  return_fit adds int64
    (h, w, 3): the determinants D, Da, Db of the fit - the gradient is (Da / D, Db / D) slabs per cell -, zeros where a cell has no fit;
    return_counts adds (unknown, traversable, BODY, STEP only, SLOPE only).  Pure host code: needs no GPU."""
    return _traversability_from_columns(columns, rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, slope)


def traversability_rough_from_columns(columns, step_slabs, robot_slabs, slope, rough, rect=None, return_ground=False, return_fit=False, return_counts=False):
    """kicp_elev_traversability_rough_from_columns: traversability_slope_from_columns with the class ROUGH - a cell with a fit is also an
    obstacle when the mean squared residual of its fit set to the fitted plane exceeds rough.num / rough.den slabs^2 (include/kicp.h
    states Q).  rough: an ElevationRoughConfig, or (num, den), or a dict.  return_fit adds int64 (h, w, 5): D, Da, Db, Q, n - the mean
    squared residual is Q / (n D) -, zeros where a cell has no fit; return_counts adds (unknown, traversable, BODY, STEP only, SLOPE
    only, ROUGH only).  Pure host code: needs no GPU."""
    return _traversability_from_columns(columns, rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, slope, rough)


def elev_slope_limit(cell, slab, max_tangent):
    """kicp_elev_slope_limit: -> (rise_slabs, run_cells) of the slope limit whose tangent is max_tangent on cells of side `cell` and
    slabs of `slab` metres: run_cells = 1024, rise_slabs = floor(max_tangent * cell / slab * 1024)"""
    cfg, rise, run = ElevationConfig(float(cell), 0.0, 0.0, 0, 0, 0.0, float(slab), 0.0), C.c_uint(), C.c_uint()
    _check(lib().kicp_elev_slope_limit(C.byref(cfg), float(max_tangent), C.byref(rise), C.byref(run)))
    return rise.value, run.value


def elev_rough_limit(slab, rms_metres):
    """kicp_elev_rough_limit: -> (num, den) of the ROUGH limit whose r.m.s. residual is rms_metres on slabs of `slab` metres: den = 1024,
    num = floor((rms_metres / slab)^2 * 1024)"""
    cfg, num, den = ElevationConfig(0.0, 0.0, 0.0, 0, 0, 0.0, float(slab), 0.0), C.c_uint(), C.c_uint()
    _check(lib().kicp_elev_rough_limit(C.byref(cfg), float(rms_metres), C.byref(num), C.byref(den)))
    return num.value, den.value


def elev_update_columns(config, columns, frame, pose, sensor_xyz=(0.0, 0.0, 0.0), margin_steps=2, widen_slabs=1, keep_ground=1):
    """kicp_elev_update_columns: ElevationLayer.update as pure host code.  config: an ElevationConfig, or a dict with its fields;
    columns: uint64 (height, width), contiguous, CHANGED IN PLACE -> the nine words of the update.  Needs no GPU."""
    cfg = config if isinstance(config, ElevationConfig) else ElevationConfig(*[config[name] for name, _ in ElevationConfig._fields_])
    if not (isinstance(columns, np.ndarray) and columns.dtype == np.uint64 and columns.flags.c_contiguous and columns.flags.writeable):
        raise KicpError(KICP_ERR_ARG, "columns must be a writeable contiguous uint64 array")
    carve, out = ElevationCarveConfig(int(margin_steps), int(widen_slabs), int(keep_ground)), np.zeros(9, dtype=np.uint64)
    _check(lib().kicp_elev_update_columns(C.byref(cfg), _u64(columns), columns.size, *_frame_args(pose, sensor_xyz, frame=frame), C.byref(carve), _u64(out)))
    return tuple(int(v) for v in out)


class ElevationLayer(Handle):
    """kicp_elev: a world-aligned layer over a grid's geometry that keeps, per cell, one 64-bit column of the world heights that ever
    returned there, and reads traversability off it by height over the local ground (include/kicp.h states the exact semantics and the
    known limitations).  integrate only ever sets bits; update also clears the bits a frame's rays pass through, so what has left is
    forgotten.  It owns its device memory; the columns stay in HBM until they are asked for."""

    _destroy = "kicp_elev_destroy"

    def __init__(self, cell, origin_x, origin_y, width, height, z_origin, slab, max_ray, device=0):
        cfg = ElevationConfig(float(cell), float(origin_x), float(origin_y), int(width), int(height), float(z_origin), float(slab), float(max_ray))
        self._create("kicp_elev_create", C.byref(cfg), int(device))
        self.device, self.width, self.height = device, int(width), int(height)
        self._last, self._last_update = np.zeros(6, dtype=np.uint64), np.zeros(9, dtype=np.uint64)

    def info(self):
        """-> dict: the configuration's fields, reach (cells) and frames (integrated since creation or clear)"""
        return _info("kicp_elev_info", self._h, ElevationConfig(), reach=C.c_int(), frames=C.c_ulonglong())

    def clear(self):
        _check(lib().kicp_elev_clear(self._h))

    def integrate(self, frame, pose, sensor_xyz=(0.0, 0.0, 0.0)):
        """kicp_elev_integrate: one frame of points in the base frame (host memory) at `pose`, the sensor at `sensor_xyz` in the base frame
        -> (used, skipped, outside_grid, outside_column, new_bits, new_cells)"""
        _check(lib().kicp_elev_integrate(self._h, *_frame_args(pose, sensor_xyz, frame=frame), _u64(self._last)))
        return self.last_frame()

    def integrate_device(self, device_frame, pose, sensor_xyz=(0.0, 0.0, 0.0), n=None):
        """kicp_elev_integrate_device: the same for a DeviceFrame (or anything with .ptr and .n) already in HBM"""
        _check(lib().kicp_elev_integrate_device(self._h, *_frame_args(pose, sensor_xyz, device_frame=device_frame, n=n), _u64(self._last)))
        return self.last_frame()

    def _update(self, entry, frame_args, margin_steps, widen_slabs, keep_ground):
        """what update and update_device share"""
        cfg, out = ElevationCarveConfig(int(margin_steps), int(widen_slabs), int(keep_ground)), np.zeros(9, dtype=np.uint64)
        _check(entry(self._h, *frame_args, C.byref(cfg), _u64(out)))
        self._last[:], self._last_update = out[:6], out
        return self.last_update()

    def update(self, frame, pose, sensor_xyz=(0.0, 0.0, 0.0), margin_steps=2, widen_slabs=1, keep_ground=1):
        """kicp_elev_update: the frame as an UPDATE - the bits its rays pass through are cleared (the last margin_steps steps of a ray
        left alone, each step's slabs widened by widen_slabs, a column's lowest bit kept with keep_ground), then the frame is marked as
        integrate marks it -> integrate's six words, counted on the carved columns, then (carve_points, bits_cleared, cells_emptied)"""
        return self._update(lib().kicp_elev_update, _frame_args(pose, sensor_xyz, frame=frame), margin_steps, widen_slabs, keep_ground)

    def update_device(self, device_frame, pose, sensor_xyz=(0.0, 0.0, 0.0), margin_steps=2, widen_slabs=1, keep_ground=1, n=None):
        """kicp_elev_update_device: the same for a DeviceFrame (or anything with .ptr and .n) already in HBM"""
        return self._update(lib().kicp_elev_update_device, _frame_args(pose, sensor_xyz, device_frame=device_frame, n=n), margin_steps, widen_slabs,
                            keep_ground)

    def last_frame(self):
        """(used, skipped, outside_grid, outside_column, new_bits, new_cells) of the last integrated or updated frame"""
        return tuple(int(v) for v in self._last)

    def last_update(self):
        """the nine words of the last update (zeros before the first one): last_frame()'s six, then carve_points, bits_cleared,
        cells_emptied"""
        return tuple(int(v) for v in self._last_update)

    def columns(self):
        """-> uint64 (height, width): bit b of a column is set when a return ever had a world height in slab b"""
        out = np.empty((self.height, self.width), dtype=np.uint64)
        _check(lib().kicp_elev_columns(self._h, _u64(out), out.size))
        return out

    def set_columns(self, columns):
        c = np.ascontiguousarray(columns, dtype=np.uint64)
        _check(lib().kicp_elev_set_columns(self._h, _u64(c), c.size))

    def scroll(self, dx, dy):
        """kicp_elev_scroll: OccupancyGrid.scroll for the columns: the window moves by (dx, dy) cells on the GPU, columns that enter are
        zero, the origin becomes origin + d * cell and the last window is translated.  A planner grid fed by to_grid* is scrolled by
        the same (dx, dy) by its owner."""
        _check(lib().kicp_elev_scroll(self._h, int(dx), int(dy)))

    def follow(self, x, y, margin, step):
        """kicp_elev_follow: OccupancyGrid.follow for the layer -> the (dx, dy) applied"""
        dx, dy = C.c_int(), C.c_int()
        _check(lib().kicp_elev_follow(self._h, float(x), float(y), int(margin), int(step), C.byref(dx), C.byref(dy)))
        return int(dx.value), int(dy.value)

    def last_window(self):
        """kicp_elev_last_window: (x0, y0, w, h) of the last integrated frame's window clipped to the layer, by OccupancyGrid.last_window's
        rules; that rectangle grown by one cell is all a frame can change of the traversability"""
        return _last_window("kicp_elev_last_window", self._h)

    def _traversability(self, rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, *fit):
        """what the three traversability* methods share"""
        x0, y0, w, h = _rect(rect, self.width, self.height)
        suffix, cfgs, fit_values, count_words = _elev_classes(step_slabs, robot_slabs, *fit)
        entry = getattr(lib(), "kicp_elev_traversability" + suffix)
        return _traversability_call(lambda *outs: entry(self._h, *cfgs, x0, y0, w, h, *outs), w, h, return_ground, return_fit, return_counts, fit_values, count_words)

    def _to_grid(self, grid, step_slabs, robot_slabs, *fit):
        """what the three to_grid* methods share"""
        suffix, cfgs, _, _ = _elev_classes(step_slabs, robot_slabs, *fit)
        _check(getattr(lib(), "kicp_elev_to_grid" + suffix)(self._h, *cfgs, grid._h))

    def traversability(self, step_slabs, robot_slabs, rect=None, return_ground=False, return_counts=False):
        """kicp_elev_traversability: on the GPU, traversability_from_columns' result on the columns where they are"""
        return self._traversability(rect, return_ground, False, return_counts, step_slabs, robot_slabs)

    def to_grid(self, grid, step_slabs, robot_slabs):
        """kicp_elev_to_grid: on the GPU, the classes of every cell into the counters of `grid`, an OccupancyGrid of equal cell, origin,
        width and height on the same device that the caller dedicates to it: obstacle (1, 0), traversable (0, 1), unknown (0, 0).  At
        min_observations = 1 grid.costmap, .potential, .score_arcs, .frontiers and .gain then run on traversability."""
        self._to_grid(grid, step_slabs, robot_slabs)

    def traversability_slope(self, step_slabs, robot_slabs, slope, rect=None, return_ground=False, return_fit=False, return_counts=False):
        """kicp_elev_traversability_slope: on the GPU, traversability_slope_from_columns' result on the columns where they are; a frame
        changes it only inside last_window() grown by max(1, slope.radius_cells) cells"""
        return self._traversability(rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, slope)

    def to_grid_slope(self, grid, step_slabs, robot_slabs, slope):
        """kicp_elev_to_grid_slope: to_grid with the slope limit - a SLOPE cell is an obstacle (1, 0) like a BODY or STEP one"""
        self._to_grid(grid, step_slabs, robot_slabs, slope)

    def traversability_rough(self, step_slabs, robot_slabs, slope, rough, rect=None, return_ground=False, return_fit=False, return_counts=False):
        """kicp_elev_traversability_rough: on the GPU, traversability_rough_from_columns' result on the columns where they are; a frame
        changes it only inside last_window() grown by max(1, slope.radius_cells) cells"""
        return self._traversability(rect, return_ground, return_fit, return_counts, step_slabs, robot_slabs, slope, rough)

    def to_grid_rough(self, grid, step_slabs, robot_slabs, slope, rough):
        """kicp_elev_to_grid_rough: to_grid_slope with the class ROUGH - a ROUGH cell is an obstacle (1, 0) too"""
        self._to_grid(grid, step_slabs, robot_slabs, slope, rough)

    def rough_limit(self, rms_metres):
        """elev_rough_limit for this layer's slab -> (num, den)"""
        return elev_rough_limit(self.info()["slab"], rms_metres)

    def slope_limit(self, max_tangent):
        """elev_slope_limit for this layer's cell and slab -> (rise_slabs, run_cells)"""
        info = self.info()
        return elev_slope_limit(info["cell"], info["slab"], max_tangent)
