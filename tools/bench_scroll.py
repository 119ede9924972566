"""What a scroll costs (kicp_grid_scroll, kicp_elev_scroll) beside the floor any implementation of its contract pays: a device-to-device
copy of the same number of bytes.  tools/bench_transients.py's method: one process, the caller bound as tools/bench_pipeline.py binds
it, the host clock around each call, which returns with the stream drained; warm; the calls of every case alternate `rounds` times;
median, p10 / p90, min .. max.

Cases: grids of the four sizes of DESIGN 5j's table (1600^2, 320^2, 960^2, 192^2 cells; 4 bytes per cell) with and without a transient
plane (1 more byte per cell), and a height layer of 1600^2 (8 bytes per cell), each shifted by (step, 0), (0, step) and (step, step),
step = 64, alternating with the opposite shift so that the origin stays where it is.  Per case also:
  - the yardstick: hipMemcpyAsync device to device of the plane's bytes (for a grid with a plane: the two copies) between two buffers
    of this tool, on a non-blocking stream of its own created as the handles create theirs, and hipStreamSynchronize - timed in the
    same loop, the same way (the handle's own stream is not reachable from outside the library);
  - kicp_grid_follow / kicp_elev_follow of a position inside the band: the call that a frame usually makes.  It must cost host
    arithmetic only - far below the few microseconds any launch or synchronisation costs.
Every scroll's result is checked once against kicp_shift_plane.  Prints one JSON line.

    python tools/bench_scroll.py [--rounds 30] [--step 64] [--lib PATH-of-another-build]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kinematic_icp_amd as K  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from bench_relocalize import spread  # noqa: E402

SIDES = (1600, 320, 960, 192)
HIP_STREAM_NON_BLOCKING, HIP_MEMCPY_DEVICE_TO_DEVICE = 1, 3


class Copier:
    """the yardstick: two device buffers and a non-blocking stream through the HIP runtime the library itself is linked to - the very
    file the loader mapped for it, read off this process's map, so that a second runtime can never be the one that is timed"""

    def __init__(self, max_bytes):
        K.lib()
        with open("/proc/self/maps") as maps:
            paths = {line.split()[-1] for line in maps if "libamdhip64.so" in line}
        if len(paths) != 1:
            raise SystemExit("expected one HIP runtime in this process, found %s" % sorted(paths))
        self.hip = C.CDLL(paths.pop())
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.src, self.dst, self.stream = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for call in (lambda: self.hip.hipMalloc(C.byref(self.src), C.c_size_t(max_bytes)), lambda: self.hip.hipMalloc(C.byref(self.dst), C.c_size_t(max_bytes)),
                     lambda: self.hip.hipMemset(self.src, 1, C.c_size_t(max_bytes)), lambda: self.hip.hipStreamCreateWithFlags(C.byref(self.stream), HIP_STREAM_NON_BLOCKING)):
            if call() != 0:
                raise SystemExit("the HIP runtime refused the yardstick's set-up")

    def copy(self, pieces):
        """the pieces (bytes each) one after the other, then the wait -> milliseconds by the host clock"""
        t = time.perf_counter()
        at, rc = 0, 0
        for n in pieces:
            rc |= self.hip.hipMemcpyAsync(C.c_void_p(self.dst.value + at), C.c_void_p(self.src.value + at), n, HIP_MEMCPY_DEVICE_TO_DEVICE, self.stream)
            at += n
        rc |= self.hip.hipStreamSynchronize(self.stream)
        dt = (time.perf_counter() - t) * 1e3
        assert rc == 0
        return dt


def make_cases(step):
    rng = np.random.default_rng(7)
    out = []
    for side in SIDES:
        for with_plane in (False, True):
            grid = K.OccupancyGrid(0.05, -0.025 * side, -0.025 * side, side, side, 0.1, 1.5, 1.0)
            grid.set_counts(rng.integers(0, 65536, (side, side, 2), dtype=np.uint16))
            if with_plane:  # a detection allocates the plane; what it holds does not change what a shift costs
                grid.transients(np.array([[0.1, 0.1, 0.5]]), np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]))
            out.append({"what": "grid" + (" + transient plane" if with_plane else ""), "side": side, "handle": grid, "pieces": [4 * side * side] + ([side * side] if with_plane else []),
                        "read": grid.counts, "scroll": K.lib().kicp_grid_scroll, "follow": K.lib().kicp_grid_follow})
    side = SIDES[0]
    layer = K.ElevationLayer(0.05, -0.025 * side, -0.025 * side, side, side, -1.0, 0.0625, 1.0)
    layer.set_columns(rng.integers(0, 1 << 63, (side, side), dtype=np.uint64))
    out.append({"what": "height layer", "side": side, "handle": layer, "pieces": [8 * side * side], "read": layer.columns, "scroll": K.lib().kicp_elev_scroll,
                "follow": K.lib().kicp_elev_follow})
    for c in out:
        c["shifts"] = {"(%d, 0)" % step: (step, 0), "(0, %d)" % step: (0, step), "(%d, %d)" % (step, step): (step, step)}
        c["t"] = {name: [] for name in list(c["shifts"]) + ["copy", "follow_no_scroll"]}
        for dx, dy in c["shifts"].values():  # once, checked: there and back leaves what neither shift dropped
            before = c["read"]()
            assert c["scroll"](c["handle"]._h, dx, dy) == 0
            assert np.array_equal(c["read"](), K.shift_plane(before, dx, dy)), (c["what"], c["side"], dx, dy)
            assert c["scroll"](c["handle"]._h, -dx, -dy) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--lib", default=None, help="another build of the library to load instead (an A/B of the kernel)")
    a = ap.parse_args()
    if a.lib:
        K.LIB_PATH = os.path.abspath(a.lib)
    bind, where = placement()
    if bind:
        bind()
    todo = make_cases(a.step)
    copier = Copier(max(sum(c["pieces"]) for c in todo))
    dx, dy = C.c_int(), C.c_int()
    for r in range(a.rounds + 3):  # (the first three rounds warm)
        for c in todo:
            h, t = c["handle"]._h, {}
            for name, (sx, sy) in c["shifts"].items():
                t0 = time.perf_counter()
                rc = c["scroll"](h, sx, sy)
                t[name] = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and c["scroll"](h, -sx, -sy) == 0
            t["copy"] = copier.copy(c["pieces"])
            t0 = time.perf_counter()
            rc = c["follow"](h, 0.0, 0.0, 8, a.step, C.byref(dx), C.byref(dy))  # the origin is minus half the side: (0, 0) is the middle cell
            t["follow_no_scroll"] = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and (dx.value, dy.value) == (0, 0)
            if r >= 3:
                for name, v in t.items():
                    c["t"][name].append(v)
    out = [{"what": c["what"], "cells": [c["side"], c["side"]], "bytes_shifted": int(sum(c["pieces"])), "launches": len(c["pieces"]),
            **{("scroll_%s_ms" % name if name in c["shifts"] else name + "_ms"): spread(v) for name, v in c["t"].items()}} for c in todo]
    print(json.dumps({"caller_process": where, "rounds": a.rounds, "step_cells": a.step, "library": a.lib or "the tree's", "scroll": out}))


if __name__ == "__main__":
    main()
