"""What the height columns cost (kicp_elev_*), one process, the caller bound as tools/bench_pipeline.py binds it.

Cases: tools/bench_grid.py's - a 131 072-point frame (64 beams x 2048 azimuths) in cfg1's scene and a 1 080-beam scan in cfg4's, each at
0.05 m and 0.25 m cells; slabs of 0.125 m from 1 m below the floor.  The host clock around each call, which returns after its kernels
have completed.  Warm; everything that is compared alternates in the same process `rounds` times; median, p10 / p90, min .. max.
  - integrate: kicp_elev_integrate_device of the frame onto an EMPTY layer (cleared before, untimed: every bit is new, all atomics) and
    of the SAME frame again (steady state: no new bit), and kicp_grid_integrate_device on a grid of the same geometry as the yardstick;
    with --ab NAME=LIBRARY (repeatable) the same two calls through another build of the library loaded beside this one - how a kernel
    variant is compared before the loser is deleted;
  - traversability: kicp_elev_traversability of a full 1 600 x 1 600 layer and of its last window grown by one cell (max_ray 12 m there,
    so that the window is not the whole layer), the full layer once more with the ground bytes and the four counts, and
    kicp_grid_occupancy of an equal grid as the yardstick; kicp_elev_to_grid too;
  - with --pipeline: KinematicICP::RegisterFrame on a short drive in the case's scene (tests/cpp/elev_facade_test, mode `timed`; the
    frames as vectors, the clock around the call), a process with the layer and a process without, alternating `pipeline-rounds`
    times; with --contender NAME=EXECUTABLE:LIBDIR (repeatable) also a process of another build's `<facade test> timed .. off` - the
    parent commit's, to show that a disabled layer costs nothing: the median of the drive's second half per process, then median and
    min .. max over the processes.
  - with --carve INSTEAD of the above: kicp_elev_update_device (margin_steps 2, widen_slabs 1, keep_ground set) of the frame onto an
    EMPTY layer (nothing to clear: the rays are walked, every lane loads and no atomic AND is issued) and of the SAME frame again
    (steady state), beside kicp_elev_integrate_device of the same frame again and kicp_grid_integrate_device - the yardsticks, the
    grid walks the same rays once per HIT cell - from the same process, alternating; --ab compares another build's update; with
    --pipeline the drive through tests/cpp/elev_carve_facade_test, mode `timed`: a process without a layer, one with a layer and one
    with a layer that carves, and per --contender a process of another build's tests/cpp/elev_facade_test `timed .. on` - the parent
    commit's pipeline with its layer, which is what this build's frame must cost while carving is off.
  - with --slope INSTEAD of the above: the slope limit (kicp_elev_traversability_slope, kicp_elev_to_grid_slope) on the traversability
    case's 1 600 x 1 600 layer at L = 2, 4 and 8 - the full layer, the last window grown by L, the full layer with every optional
    output, and into a grid - beside kicp_elev_traversability and kicp_elev_to_grid of this build and, with --ab parent=LIBRARY, of
    the parent commit's library on the same columns, alternating (raw output kept as profiles/elev_slope_bench.json).
  - with --rough INSTEAD of the above: the class ROUGH (kicp_elev_traversability_rough, kicp_elev_to_grid_rough) at L = 2, 4 and 8 on that
    sparse layer and on a fully known one of the same size, beside the slope limit's and the plain calls of this build and, with
    --ab parent=LIBRARY (twice, two builds of the parent commit: the spread between them is the yardstick), all three of the parent's
    where it has them, on the same columns, alternating; with --fill also kicp_grid_fill_unknown of the grid kicp_elev_to_grid wrote from the mapping grid of
    the same frame, beside kicp_elev_to_grid (raw output kept as profiles/elev_rough_bench.json).
Prints one JSON line.

    python tools/bench_elev.py [--rounds 30] [--carve | --slope | --rough [--fill]] [--ab NAME=LIB] [--pipeline] [--pipeline-rounds 3] [--pipeline-frames 16] [--contender NAME=EXE:LIBDIR]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kinematic_icp_amd as K  # noqa: E402
from kinematic_icp_amd import synthetic as syn  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from bench_relocalize import spread  # noqa: E402
from bench_grid import CELLS, GEOMETRY, grid_config, make_grid, scene_and_beams  # noqa: E402

Z_ORIGIN, SLAB = -1.0, 0.125
STEP_SLABS, ROBOT_SLABS = 2, 12
CARVE = (2, 1, 1)  # margin_steps, widen_slabs, keep_ground


class RawLayer:
    """a layer of another build of the library (an --ab contender), through its C-ABI"""

    def __init__(self, lib, cfg):
        self.lib, self._h = lib, C.c_void_p()
        c = K.ElevationConfig(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], Z_ORIGIN, SLAB, cfg["max_ray"])
        assert lib.kicp_elev_create(C.byref(c), 0, C.byref(self._h)) == 0
        self._last = np.zeros(6, dtype=np.uint64)

    def clear(self):
        assert self.lib.kicp_elev_clear(self._h) == 0

    def integrate_device(self, dev, pose, sensor):
        rc = self.lib.kicp_elev_integrate_device(self._h, dev.ptr, dev.n, pose.ctypes.data_as(K._dp), sensor.ctypes.data_as(K._dp), self._last.ctypes.data_as(C.POINTER(C.c_ulonglong)))
        assert rc == 0
        return tuple(int(v) for v in self._last)

    def update_device(self, dev, pose, sensor, margin_steps, widen_slabs, keep_ground):
        carve, out = K.ElevationCarveConfig(margin_steps, widen_slabs, keep_ground), np.zeros(9, dtype=np.uint64)
        rc = self.lib.kicp_elev_update_device(self._h, dev.ptr, dev.n, pose.ctypes.data_as(K._dp), sensor.ctypes.data_as(K._dp), C.byref(carve), out.ctypes.data_as(C.POINTER(C.c_ulonglong)))
        assert rc == 0
        return tuple(int(v) for v in out)

    def __del__(self):
        self.lib.kicp_elev_destroy(self._h)


def load_contender(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in K._SIGNATURES.items():
        if name.startswith("kicp_elev_") or name in ("kicp_grid_create", "kicp_grid_destroy"):
            fn = getattr(lib, name, None)  # (an older build lacks the newer entries)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
    return lib


class RawClasses:
    """kicp_elev_traversability and kicp_elev_to_grid of another build (an --ab contender) on given columns: a layer and a grid of that
    build, through its C-ABI"""

    def __init__(self, lib, cfg, columns):
        self.lib, self._h, self._g = lib, C.c_void_p(), C.c_void_p()
        c = K.ElevationConfig(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], Z_ORIGIN, SLAB, cfg["max_ray"])
        g = K.GridConfig(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_min"], cfg["z_max"], cfg["max_ray"])
        assert lib.kicp_elev_create(C.byref(c), 0, C.byref(self._h)) == 0 and lib.kicp_grid_create(C.byref(g), 0, C.byref(self._g)) == 0
        assert lib.kicp_elev_set_columns(self._h, columns.ctypes.data_as(C.POINTER(C.c_ulonglong)), columns.size) == 0
        self.cfg, self.out = K.ElevationTraversabilityConfig(STEP_SLABS, ROBOT_SLABS), np.empty((cfg["height"], cfg["width"]), dtype=np.int8)

    def traversability(self):
        h, w = self.out.shape
        assert self.lib.kicp_elev_traversability(self._h, C.byref(self.cfg), 0, 0, w, h, self.out.ctypes.data_as(C.POINTER(C.c_byte)), None, None, self.out.size) == 0
        return self.out

    def to_grid(self):
        assert self.lib.kicp_elev_to_grid(self._h, C.byref(self.cfg), self._g) == 0

    def traversability_slope(self, slope):
        h, w = self.out.shape
        scfg = K.ElevationSlopeConfig(*slope)
        assert self.lib.kicp_elev_traversability_slope(self._h, C.byref(self.cfg), C.byref(scfg), 0, 0, w, h, self.out.ctypes.data_as(C.POINTER(C.c_byte)), None, None, None,
                                                       self.out.size) == 0
        return self.out

    def to_grid_slope(self, slope):
        scfg = K.ElevationSlopeConfig(*slope)
        assert self.lib.kicp_elev_to_grid_slope(self._h, C.byref(self.cfg), C.byref(scfg), self._g) == 0

    def traversability_rough(self, slope, rough):
        h, w = self.out.shape
        scfg, rcfg = K.ElevationSlopeConfig(*slope), K.ElevationRoughConfig(*rough)
        assert self.lib.kicp_elev_traversability_rough(self._h, C.byref(self.cfg), C.byref(scfg), C.byref(rcfg), 0, 0, w, h, self.out.ctypes.data_as(C.POINTER(C.c_byte)), None,
                                                       None, None, self.out.size) == 0
        return self.out

    def to_grid_rough(self, slope, rough):
        scfg, rcfg = K.ElevationSlopeConfig(*slope), K.ElevationRoughConfig(*rough)
        assert self.lib.kicp_elev_to_grid_rough(self._h, C.byref(self.cfg), C.byref(scfg), C.byref(rcfg), self._g) == 0

    def __del__(self):
        lib = getattr(self, "lib", None)
        if lib is None:
            return
        if getattr(self, "_h", None):
            lib.kicp_elev_destroy(self._h)
            self._h = None
        if getattr(self, "_g", None):
            lib.kicp_grid_destroy(self._g)
            self._g = None


def make_layer(cfg):
    return K.ElevationLayer(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], Z_ORIGIN, SLAB, cfg["max_ray"])


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def integrate_rows(rounds, contenders):
    cases = []
    for name in GEOMETRY:
        cfg, scene, dirs, rng = scene_and_beams(name)
        pose = syn.planar_pose(1.2, -0.7, 0.9)
        frame = np.ascontiguousarray(syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng))
        sensor = np.array([0.0, 0.0, cfg.sensor_height])
        for cell in CELLS:
            gcfg = grid_config(name, cell)
            layers = {"this": make_layer(gcfg)}
            layers.update({who: RawLayer(lib, gcfg) for who, lib in contenders.items()})
            cases.append(dict(name=name, cell=cell, cfg=gcfg, layers=layers, grid=make_grid(gcfg), frame=frame, dev=K.DeviceFrame(frame), pose=pose, sensor=sensor,
                              t_grid=[], t_first={w: [] for w in layers}, t_again={w: [] for w in layers}, stats={}))
    for r in range(rounds + 3):  # (the first three rounds warm)
        for c in cases:
            t_grid, _ = timed(lambda: c["grid"].integrate_device(c["dev"], c["pose"], c["sensor"]))
            if r >= 3:
                c["t_grid"].append(t_grid)
            for who, layer in c["layers"].items():
                layer.clear()
                t_first, first = timed(lambda: layer.integrate_device(c["dev"], c["pose"], c["sensor"]))
                t_again, again = timed(lambda: layer.integrate_device(c["dev"], c["pose"], c["sensor"]))
                assert again[:4] == first[:4] and again[4:] == (0, 0) and c["stats"].setdefault("first", first) == first  # every build computes the same
                if r >= 3:
                    c["t_first"][who].append(t_first), c["t_again"][who].append(t_again)
    rows = []
    for c in cases:
        first = c["stats"]["first"]
        row = {"scene": c["name"], "points": len(c["frame"]), "cell_m": c["cell"], "layer_cells": [c["cfg"]["width"], c["cfg"]["height"]], "reach_cells": c["cfg"]["reach"],
               "used": first[0], "skipped": first[1], "outside_grid": first[2], "outside_column": first[3], "bits_of_the_frame": first[4], "cells_of_the_frame": first[5],
               "grid_integrate_device_ms": spread(c["t_grid"])}
        for who in c["layers"]:
            row["elev_first_frame_ms_" + who] = spread(c["t_first"][who])
            row["elev_same_frame_again_ms_" + who] = spread(c["t_again"][who])
        rows.append(row)
    return rows


def carve_rows(rounds, contenders):
    """the update beside the two yardsticks, on integrate_rows' frames and cells"""
    cases = []
    for name in GEOMETRY:
        cfg, scene, dirs, rng = scene_and_beams(name)
        pose = syn.planar_pose(1.2, -0.7, 0.9)
        frame = np.ascontiguousarray(syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng))
        sensor = np.array([0.0, 0.0, cfg.sensor_height])
        for cell in CELLS:
            gcfg = grid_config(name, cell)
            layers = {"this": make_layer(gcfg)}
            layers.update({who: RawLayer(lib, gcfg) for who, lib in contenders.items()})
            cases.append(dict(name=name, cell=cell, cfg=gcfg, layers=layers, grid=make_grid(gcfg), frame=frame, dev=K.DeviceFrame(frame), pose=pose, sensor=sensor,
                              t_grid=[], t_integrate=[], t_first={w: [] for w in layers}, t_again={w: [] for w in layers}, stats={}))
    for r in range(rounds + 3):  # (the first three rounds warm)
        for c in cases:
            t_grid, _ = timed(lambda: c["grid"].integrate_device(c["dev"], c["pose"], c["sensor"]))
            for who, layer in c["layers"].items():
                layer.clear()
                t_first, first = timed(lambda: layer.update_device(c["dev"], c["pose"], c["sensor"], *CARVE))
                t_again, again = timed(lambda: layer.update_device(c["dev"], c["pose"], c["sensor"], *CARVE))
                assert first[7:] == (0, 0) and again[:4] == first[:4] and again[6] == first[6]
                assert c["stats"].setdefault("first", first) == first and c["stats"].setdefault("again", again) == again  # every build computes the same
                if r >= 3:
                    c["t_first"][who].append(t_first), c["t_again"][who].append(t_again)
            t_integrate, _ = timed(lambda: c["layers"]["this"].integrate_device(c["dev"], c["pose"], c["sensor"]))
            if r >= 3:
                c["t_grid"].append(t_grid), c["t_integrate"].append(t_integrate)
    rows = []
    for c in cases:
        first, again = c["stats"]["first"], c["stats"]["again"]
        row = {"scene": c["name"], "points": len(c["frame"]), "cell_m": c["cell"], "layer_cells": [c["cfg"]["width"], c["cfg"]["height"]], "reach_cells": c["cfg"]["reach"],
               "margin_steps": CARVE[0], "widen_slabs": CARVE[1], "keep_ground": CARVE[2], "used": first[0], "carve_points": first[6],
               "bits_cleared_same_frame_again": again[7], "new_bits_same_frame_again": again[4],
               "grid_integrate_device_ms": spread(c["t_grid"]), "elev_integrate_device_same_frame_again_ms": spread(c["t_integrate"])}
        for who in c["layers"]:
            row["elev_update_first_frame_ms_" + who] = spread(c["t_first"][who])
            row["elev_update_same_frame_again_ms_" + who] = spread(c["t_again"][who])
        rows.append(row)
    return rows


def traversability_rows(rounds):
    name = "cfg1"
    cfg, scene, dirs, rng = scene_and_beams(name)
    pose = syn.planar_pose(1.2, -0.7, 0.9)
    frame = np.ascontiguousarray(syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng))
    sensor = np.array([0.0, 0.0, cfg.sensor_height])
    gcfg = dict(grid_config(name, 0.05), max_ray=12.0, reach=240)
    layer, grid, other = make_layer(gcfg), make_grid(gcfg), make_grid(gcfg)
    layer.integrate(frame, pose, sensor), grid.integrate(frame, pose, sensor)
    x0, y0, w, h = layer.last_window()
    ax, ay = max(x0 - 1, 0), max(y0 - 1, 0)
    rect = (ax, ay, min(x0 + w + 1, gcfg["width"]) - ax, min(y0 + h + 1, gcfg["height"]) - ay)
    t = {"full": [], "counted": [], "window": [], "occupancy": [], "to_grid": []}
    for r in range(rounds + 3):
        a, full = timed(lambda: layer.traversability(STEP_SLABS, ROBOT_SLABS))
        b, part = timed(lambda: layer.traversability(STEP_SLABS, ROBOT_SLABS, rect=rect))
        c, _ = timed(lambda: grid.occupancy(1))
        d, _ = timed(lambda: layer.to_grid(other, STEP_SLABS, ROBOT_SLABS))
        e, _ = timed(lambda: layer.traversability(STEP_SLABS, ROBOT_SLABS, return_ground=True, return_counts=True))
        if r >= 3:
            t["full"].append(a), t["window"].append(b), t["occupancy"].append(c), t["to_grid"].append(d), t["counted"].append(e)
    assert np.array_equal(part, full[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]) and np.array_equal(other.occupancy(1), full)
    counts = layer.traversability(STEP_SLABS, ROBOT_SLABS, return_counts=True)[1]
    return [{"scene": name, "points": len(frame), "cell_m": 0.05, "layer_cells": [gcfg["width"], gcfg["height"]], "window_grown_by_one": list(rect),
             "step_slabs": STEP_SLABS, "robot_slabs": ROBOT_SLABS, "unknown_traversable_body_step": list(counts), "traversability_full_ms": spread(t["full"]), "traversability_full_with_ground_and_counts_ms": spread(t["counted"]),
             "traversability_window_ms": spread(t["window"]), "grid_occupancy_full_ms": spread(t["occupancy"]), "to_grid_ms": spread(t["to_grid"])}]


SLOPE_RADII = (2, 4, 8)


def slope_rows(rounds, contenders):
    """the slope limit on traversability_rows' 1 600 x 1 600 layer, at L = 2, 4 and 8 (K = (S + 1) L, min_cells 12, 20 degrees): the full
    layer, the last window grown by L, the full layer with ground bytes, determinants and counts, and kicp_elev_to_grid_slope - beside
    kicp_elev_traversability and kicp_elev_to_grid of this build and of every --ab contender (the parent commit's library), on the
    same columns, alternating"""
    name = "cfg1"
    cfg, scene, dirs, rng = scene_and_beams(name)
    pose = syn.planar_pose(1.2, -0.7, 0.9)
    frame = np.ascontiguousarray(syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng))
    sensor = np.array([0.0, 0.0, cfg.sensor_height])
    gcfg = dict(grid_config(name, 0.05), max_ray=12.0, reach=240)
    layer, other = make_layer(gcfg), make_grid(gcfg)
    layer.integrate(frame, pose, sensor)
    columns = layer.columns()
    raws = {who: RawClasses(lib, gcfg, columns) for who, lib in contenders.items()}
    x0, y0, w, h = layer.last_window()
    rise, run = layer.slope_limit(np.tan(np.deg2rad(20.0)))
    slopes = {L: (L, (STEP_SLABS + 1) * L, 12, rise, run) for L in SLOPE_RADII}
    rects = {L: (max(x0 - L, 0), max(y0 - L, 0), min(x0 + w + L, gcfg["width"]) - max(x0 - L, 0), min(y0 + h + L, gcfg["height"]) - max(y0 - L, 0)) for L in SLOPE_RADII}
    t = {"traversability_full_ms_this": [], "to_grid_ms_this": []}
    for who in raws:
        t["traversability_full_ms_" + who], t["to_grid_ms_" + who] = [], []
    for L in SLOPE_RADII:
        for what in ("slope_full", "slope_window", "slope_full_with_ground_fit_and_counts", "to_grid_slope"):
            t["%s_ms_L%d" % (what, L)] = []
    results = {}
    for r in range(rounds + 3):  # (the first three rounds warm)
        now = {}
        now["traversability_full_ms_this"], plain = timed(lambda: layer.traversability(STEP_SLABS, ROBOT_SLABS))
        now["to_grid_ms_this"], _ = timed(lambda: layer.to_grid(other, STEP_SLABS, ROBOT_SLABS))
        for who, raw in raws.items():
            now["traversability_full_ms_" + who], theirs = timed(raw.traversability)
            now["to_grid_ms_" + who], _ = timed(raw.to_grid)
            assert np.array_equal(theirs, plain)  # every build computes the same
        for L in SLOPE_RADII:
            now["slope_full_ms_L%d" % L], full = timed(lambda: layer.traversability_slope(STEP_SLABS, ROBOT_SLABS, slopes[L]))
            now["slope_window_ms_L%d" % L], part = timed(lambda: layer.traversability_slope(STEP_SLABS, ROBOT_SLABS, slopes[L], rect=rects[L]))
            now["slope_full_with_ground_fit_and_counts_ms_L%d" % L], counted = timed(
                lambda: layer.traversability_slope(STEP_SLABS, ROBOT_SLABS, slopes[L], return_ground=True, return_fit=True, return_counts=True))
            now["to_grid_slope_ms_L%d" % L], _ = timed(lambda: layer.to_grid_slope(other, STEP_SLABS, ROBOT_SLABS, slopes[L]))
            rx, ry, rw, rh = rects[L]
            assert np.array_equal(part, full[ry:ry + rh, rx:rx + rw]) and np.array_equal(counted[0], full) and np.array_equal(other.occupancy(1), full)
            assert np.array_equal(full[full != plain], np.full(int((full != plain).sum()), 100, dtype=np.int8)) and counted[3][4] == int((full != plain).sum())
            results[L] = counted[3]
        if r >= 3:
            for key, ms in now.items():
                t[key].append(ms)
    row = {"scene": name, "points": len(frame), "cell_m": 0.05, "slab_m": SLAB, "layer_cells": [gcfg["width"], gcfg["height"]], "step_slabs": STEP_SLABS, "robot_slabs": ROBOT_SLABS,
           "slope_configs_L_K_min_rise_run": [list(slopes[L]) for L in SLOPE_RADII], "windows_grown_by_L": [list(rects[L]) for L in SLOPE_RADII],
           "unknown_traversable_body_step_slope": {"L%d" % L: list(results[L]) for L in SLOPE_RADII}}
    row.update({key: spread(v) for key, v in t.items()})
    return [row]


ROUGH_LIMIT = (512, 1024)  # half a slab^2


def known_columns(width, height):
    """a fully known layer: one bit per column, the ground rising by a slab every 64 cells in x under two slabs of noise"""
    rng = np.random.default_rng(5)
    ground = 4 + np.arange(width)[None, :] // 64 + rng.integers(0, 3, (height, width))
    return (np.uint64(1) << ground.astype(np.uint64)).astype(np.uint64)


def rough_rows(rounds, contenders, fill):
    """ROUGH (kicp_elev_traversability_rough, kicp_elev_to_grid_rough) at L = 2, 4 and 8 on slope_rows' sparse 1 600 x 1 600 layer and on
    a fully known one of that size, beside kicp_elev_traversability_slope / kicp_elev_to_grid_slope and the plain calls, each of this
    build and of every --ab contender that has the entry (the parent commit's library, built twice: the spread between the two is the
    yardstick for this build's existing calls), on the same columns, alternating.  With --fill also kicp_grid_fill_unknown of the grid kicp_elev_to_grid
    wrote, from the mapping grid of the same frame, without and with the seven counts, beside kicp_elev_to_grid as its yardstick."""
    name = "cfg1"
    cfg, scene, dirs, rng = scene_and_beams(name)
    pose = syn.planar_pose(1.2, -0.7, 0.9)
    frame = np.ascontiguousarray(syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng))
    sensor = np.array([0.0, 0.0, cfg.sensor_height])
    gcfg = dict(grid_config(name, 0.05), max_ray=12.0, reach=240)
    mapping = make_grid(gcfg)
    mapping.integrate(frame, pose, sensor)
    rows = []
    for kind in ("sparse", "known"):
        layer, other = make_layer(gcfg), make_grid(gcfg)
        if kind == "sparse":
            layer.integrate(frame, pose, sensor)
        else:
            layer.set_columns(known_columns(gcfg["width"], gcfg["height"]))
        columns = layer.columns()
        # EVERY build through the same caller, this one too: RawClasses on a preallocated output (K.ElevationLayer's methods allocate
        # theirs per call, which costs about a tenth of a plain call at this size)
        raws = {"this": RawClasses(K.lib(), gcfg, columns)}
        raws.update({who: RawClasses(lib, gcfg, columns) for who, lib in contenders.items()})
        rise, run = layer.slope_limit(np.tan(np.deg2rad(20.0)))
        slopes = {L: (L, (STEP_SLABS + 1) * L, 12, rise, run) for L in SLOPE_RADII}
        t, results, fills = {}, {}, None
        for r in range(rounds + 3):  # (the first three rounds warm)
            now, plain = {}, None
            turn = list(raws.items())[r % len(raws):] + list(raws.items())[:r % len(raws)]  # the builds take turns at going first
            for who, raw in turn:
                now["traversability_full_ms_" + who], theirs = timed(raw.traversability)
                now["to_grid_ms_" + who], _ = timed(raw.to_grid)
                plain = theirs.copy() if plain is None else plain
                assert np.array_equal(theirs, plain)  # every build computes the same
            if fill:
                layer.to_grid(other, STEP_SLABS, ROBOT_SLABS)
                now["fill_unknown_ms"], _ = timed(lambda: other.fill_unknown(mapping))
                layer.to_grid(other, STEP_SLABS, ROBOT_SLABS)
                now["fill_unknown_with_counts_ms"], fills = timed(lambda: other.fill_unknown(mapping, return_counts=True))
            for L in SLOPE_RADII:
                steep = None
                for who, raw in turn:
                    now["slope_full_ms_L%d_%s" % (L, who)], theirs = timed(lambda: raw.traversability_slope(slopes[L]))
                    now["to_grid_slope_ms_L%d_%s" % (L, who)], _ = timed(lambda: raw.to_grid_slope(slopes[L]))
                    steep = theirs.copy() if steep is None else steep
                    assert np.array_equal(theirs, steep)
                full = None
                for who, raw in turn:
                    if not hasattr(raw.lib, "kicp_elev_traversability_rough"):  # (a contender from before ROUGH)
                        continue
                    now["rough_full_ms_L%d_%s" % (L, who)], theirs = timed(lambda: raw.traversability_rough(slopes[L], ROUGH_LIMIT))
                    now["to_grid_rough_ms_L%d_%s" % (L, who)], _ = timed(lambda: raw.to_grid_rough(slopes[L], ROUGH_LIMIT))
                    full = theirs.copy() if full is None else full
                    assert np.array_equal(theirs, full)
                layer.to_grid_rough(other, STEP_SLABS, ROBOT_SLABS, slopes[L], ROUGH_LIMIT)
                now["rough_full_with_ground_fit_and_counts_ms_L%d" % L], counted = timed(
                    lambda: layer.traversability_rough(STEP_SLABS, ROBOT_SLABS, slopes[L], ROUGH_LIMIT, return_ground=True, return_fit=True, return_counts=True))
                assert np.array_equal(counted[0], full) and np.array_equal(other.occupancy(1), full)
                assert np.array_equal(full[full != steep], np.full(int((full != steep).sum()), 100, dtype=np.int8)) and counted[3][5] == int((full != steep).sum())
                results[L] = counted[3]
            if r >= 3:
                for key, ms in now.items():
                    t.setdefault(key, []).append(ms)
        row = {"scene": name, "layer": kind, "known_cells": int(np.count_nonzero(columns)), "cell_m": 0.05, "slab_m": SLAB, "layer_cells": [gcfg["width"], gcfg["height"]],
               "step_slabs": STEP_SLABS, "robot_slabs": ROBOT_SLABS, "slope_configs_L_K_min_rise_run": [list(slopes[L]) for L in SLOPE_RADII], "rough_num_den": list(ROUGH_LIMIT),
               "unknown_traversable_body_step_slope_rough": {"L%d" % L: list(results[L]) for L in SLOPE_RADII}}
        if fill:
            row["fill_kept_obstacle_kept_traversable_filled_free_filled_occupied_left_unknown_over_occupied_over_free"] = list(fills)
        row.update({key: spread(v) for key, v in t.items()})
        rows.append(row)
    return rows


def pipeline_rows(rounds, n_frames, contenders, carve=False):
    import test_elev_facade
    import test_elev_carve_facade
    exe = test_elev_carve_facade.build_binary() if carve else test_elev_facade.build_binary()
    bind, _ = placement()
    rows = []
    with tempfile.TemporaryDirectory() as td:
        for name in GEOMETRY:
            cfg, scene, dirs, rng = scene_and_beams(name)
            ext = np.concatenate([[0, 0, np.sin(0.05), np.cos(0.05)], [0.3, 0.0, cfg.sensor_height]])
            poses, drive = [syn.planar_pose(0.0, 0.0, 0.1)], os.path.join(td, name + ".bin")
            with open(drive, "wb") as fh:
                np.array([n_frames, cfg.voxel_size, cfg.max_range, 1.0]).tofile(fh)
                ext.tofile(fh)
                for k in range(n_frames):
                    delta_true = syn.planar_pose(0.2, 0.0, np.deg2rad(1.0 + 0.1 * k))
                    poses.append(syn.pose_mul(poses[-1], delta_true))
                    wl = syn.pose_mul(poses[-1], ext)
                    t = scene.raycast(wl[4:], dirs @ syn.quat_to_matrix(wl[:4]).T) + rng.normal(0, 0.01, len(dirs))
                    np.array([float(len(dirs))]).tofile(fh)
                    np.ascontiguousarray((dirs * t[:, None]).astype(np.float32).astype(np.float64)).tofile(fh)
                    np.linspace(0.0, 1.0, len(dirs)).astype(np.float32).astype(np.float64).tofile(fh)
                    syn.pose_mul(delta_true, syn.planar_pose(0.01 * (-1) ** k, 0.0, np.deg2rad(0.1))).tofile(fh)
            for cell in CELLS:
                gcfg = grid_config(name, cell)
                lfile = os.path.join(td, "layer.bin")
                # (the carve's program reads G, W, keep_ground behind the eight doubles and one more; the layer's S, H and ignores them when timed)
                np.array([gcfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height")] + [Z_ORIGIN, SLAB, gcfg["max_ray"]] +
                         (list(CARVE) if carve else [STEP_SLABS, ROBOT_SLABS]), dtype=np.float64).tofile(lfile)
                if carve:
                    runs = {"none": ([exe, "timed", drive, lfile, "none"], None, None), "carving_off": ([exe, "timed", drive, lfile, "off"], None, None),
                            "carving_on": ([exe, "timed", drive, lfile, "on"], None, None)}
                else:
                    runs = {"off": ([exe, "timed", drive, lfile, "off"], None, 0), "on": ([exe, "timed", drive, lfile, "on"], None, n_frames)}
                for who, (other_exe, libdir) in contenders.items():
                    runs[who] = ([other_exe, "timed", drive, lfile, "on" if carve else "off"], dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", "")),
                                 n_frames if carve else 0)
                per = {which: [] for which in runs}
                for r in range(rounds + 1):  # (the first round warms the file cache and the driver)
                    for which, (cmd, env, integrated) in runs.items():
                        out = subprocess.check_output(cmd, text=True, preexec_fn=bind, env=env).splitlines()
                        ms = np.array([float(ln.split()[3]) for ln in out if ln.startswith("frame ")])
                        assert integrated is None or ("frames_integrated %d" % integrated) in out
                        if r:
                            per[which].append(float(np.median(ms[len(ms) // 2:])))
                row = {"scene": name, "points": len(dirs), "cell_m": cell, "frames": n_frames,
                       "what": "median RegisterFrame wall time of the drive's second half per process; spread over %d alternating processes each" % rounds}
                row.update({"register_frame_ms_" + ("layer_" + which if which in ("on", "off", "none", "carving_on", "carving_off") else which): spread(v) for which, v in per.items()})
                rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--carve", action="store_true")
    ap.add_argument("--slope", action="store_true")
    ap.add_argument("--rough", action="store_true")
    ap.add_argument("--fill", action="store_true")
    ap.add_argument("--ab", action="append", default=[], metavar="NAME=LIB")
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--pipeline-rounds", type=int, default=3)
    ap.add_argument("--pipeline-frames", type=int, default=16)
    ap.add_argument("--contender", action="append", default=[], metavar="NAME=EXE:LIBDIR")
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    libs = {spec.split("=", 1)[0]: load_contender(spec.split("=", 1)[1]) for spec in a.ab}
    if a.rough or a.fill:
        res = {"caller_process": where, "rounds": a.rounds, "rough": rough_rows(a.rounds, libs, a.fill)}
    elif a.slope:
        res = {"caller_process": where, "rounds": a.rounds, "slope": slope_rows(a.rounds, libs)}
    elif a.carve:
        res = {"caller_process": where, "rounds": a.rounds, "carve": carve_rows(a.rounds, libs)}
    else:
        res = {"caller_process": where, "rounds": a.rounds, "integrate": integrate_rows(a.rounds, libs), "traversability": traversability_rows(a.rounds)}
    if a.pipeline:
        others = {spec.split("=", 1)[0]: tuple(os.path.abspath(p) for p in spec.split("=", 1)[1].split(":", 1)) for spec in a.contender}
        res["pipeline"] = pipeline_rows(a.pipeline_rounds, a.pipeline_frames, others, carve=a.carve)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
