"""The slope limit through the drop-in C++ headers (tests/cpp/elev_slope_facade_test.cpp): the six-frame drive of
tests/test_elev_facade.py through KinematicICP with EnableElevation, then ElevationSlopeLimit and ElevationTraversabilitySlope of the
full layer and of the last window grown by L, against the pure-host entry and the restatement on the columns the program wrote; and
the exceptions without a layer, with a bad configuration and with a bad tangent."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import clearance_ref as cr
import elev_ref as er
import elev_slope_ref as sr
from test_elev_facade import write_drive

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "elev_slope_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "elev_slope_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_elev_slope_facade_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_slope_limit_through_the_pipeline(tmp_path):
    f, g, prefix = tmp_path / "pipe.bin", tmp_path / "layer.bin", str(tmp_path / "out")
    write_drive(f)
    cfg = er.make_config(0.1, -14.0, -14.0, 300, 300, -1.0, 0.0625, 12.0)  # tests/elev_cases.py's drive layer
    S, H, L, gate, min_cells, tangent = 2, 24, 4, 12, 12, float(np.tan(np.deg2rad(20.0)))
    np.array([cfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_origin", "slab", "max_ray")] + [S, H, L, gate, min_cells, tangent],
             dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    assert "refused_without_layer 1 1" in out and "refused_bad_config 4" in out and "refused_bad_tangent 2" in out
    rise, run = sr.slope_limit(cfg["cell"], cfg["slab"], tangent)
    assert ("limit %d %d" % (rise, run)) in out and ("defaults 4 6 12 %d %d" % (rise, run)) in out and (rise, run) == (596, 1024)
    slope = (L, gate, min_cells, rise, run)
    columns = np.fromfile(prefix + "_columns.bin", dtype=np.uint64).reshape(300, 300)
    assert np.count_nonzero(columns) > 3000
    want = sr.classify(columns, S, H, slope)
    classes, ground, fit, counts = K.traversability_slope_from_columns(columns, S, H, slope, return_ground=True, return_fit=True, return_counts=True)
    assert np.array_equal(classes, want.classes) and np.array_equal(fit, want.fit) and counts == sr.counts(want)
    raw = np.fromfile(prefix + "_classes.bin", dtype=np.uint8)
    assert np.array_equal(raw[:90000].view(np.int8).reshape(300, 300), classes) and np.array_equal(raw[90000:].reshape(300, 300), ground)
    assert np.array_equal(np.fromfile(prefix + "_fit.bin", dtype=np.int64).reshape(300, 300, 3), fit)
    assert ("counts %d %d %d %d %d" % counts) in out and counts[1] > 1000 and counts[4] > 0
    window = [tuple(int(v) for v in ln.split()[1:]) for ln in out if ln.startswith("window ")][0]
    x0, y0, w, h = cr.grown(window, L, 300, 300)
    assert np.array_equal(np.fromfile(prefix + "_window.bin", dtype=np.int8).reshape(h, w), classes[y0:y0 + h, x0:x0 + w])
