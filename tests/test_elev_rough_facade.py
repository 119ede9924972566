"""The class ROUGH and the fill through the drop-in C++ headers (tests/cpp/elev_rough_facade_test.cpp): the six-frame drive of
tests/test_elev_facade.py through KinematicICP with EnableGrid and EnableElevation, then ElevationRoughLimit,
ElevationTraversabilityRough and ElevationIntoGrid in its four forms - each equal to the C calls it wraps, and to the pure-host
entries and the restatement on the columns and counters the program wrote; and the exceptions without a layer, for `rough` without
`slope`, for a fill without EnableGrid and with a bad configuration."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import elev_ref as er
import elev_rough_ref as rr
import elev_slope_ref as sr
from test_elev_facade import write_drive

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "elev_rough_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "elev_rough_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_elev_rough_facade_compiles_and_links():
    assert os.path.exists(build_binary())


def as_counters(classes):
    return np.stack([classes == 100, classes == 0], axis=-1).astype(np.uint16)


@pytest.mark.gpu
def test_rough_and_the_fill_through_the_pipeline(tmp_path):
    f, g, prefix = tmp_path / "pipe.bin", tmp_path / "layer.bin", str(tmp_path / "out")
    write_drive(f)
    cfg = er.make_config(0.1, -14.0, -14.0, 300, 300, -1.0, 0.0625, 12.0)  # tests/elev_cases.py's drive layer
    S, H, L, gate, min_cells, tangent = 2, 24, 4, 12, 12, float(np.tan(np.deg2rad(20.0)))
    rms, band, fill = cfg["slab"] * float(np.sqrt(0.5)), (-0.5, 1.5), (1, 25, 101)
    np.array([cfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_origin", "slab", "max_ray")] + [S, H, L, gate, min_cells, tangent, rms] + list(band) +
             list(fill), dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    assert "refused_without_layer 3" in out and "refused_rough_without_slope 1" in out and "refused_fill_without_grid 1" in out and "refused_bad_config 3" in out
    assert "forms_equal 4" in out  # each form of ElevationIntoGrid against the C calls it wraps
    rough = rr.rough_limit(cfg["slab"], rms)
    assert ("limit %d %d" % rough) in out and rough == (512, 1024)
    slope = (L, gate, min_cells) + sr.slope_limit(cfg["cell"], cfg["slab"], tangent)
    columns = np.fromfile(prefix + "_columns.bin", dtype=np.uint64).reshape(300, 300)
    source = np.fromfile(prefix + "_source.bin", dtype=np.uint16).reshape(300, 300, 2)
    assert np.count_nonzero(columns) > 3000 and np.count_nonzero(source[..., 1]) > 10000
    want = rr.classify(columns, S, H, slope, rough)
    classes, ground, fit, counts = K.traversability_rough_from_columns(columns, S, H, slope, rough, return_ground=True, return_fit=True, return_counts=True)
    assert np.array_equal(classes, want.classes) and np.array_equal(fit, want.fit) and counts == rr.counts(want)
    raw = np.fromfile(prefix + "_classes.bin", dtype=np.uint8)
    assert np.array_equal(raw[:90000].view(np.int8).reshape(300, 300), classes) and np.array_equal(raw[90000:].reshape(300, 300), ground)
    assert np.array_equal(np.fromfile(prefix + "_fit.bin", dtype=np.int64).reshape(300, 300, 5), fit)
    assert ("counts %d %d %d %d %d %d" % counts) in out and counts[1] > 1000 and counts[5] > 0

    def written(name):
        return np.fromfile(prefix + "_%s.bin" % name, dtype=np.uint16).reshape(300, 300, 2)

    assert np.array_equal(written("plain"), as_counters(K.traversability_from_columns(columns, S, H)))
    assert np.array_equal(written("slope"), as_counters(K.traversability_slope_from_columns(columns, S, H, slope)))
    assert np.array_equal(written("rough"), as_counters(classes))
    filled, words = K.fill_unknown_counts(as_counters(classes), source, *fill, return_counts=True)
    assert (filled, words)[1] == rr.fill(as_counters(classes), source, *fill)[1] and np.array_equal(filled, rr.fill(as_counters(classes), source, *fill)[0])
    assert np.array_equal(written("filled"), filled) and ("fill_counts %d %d %d %d %d %d %d" % words) in out and words[2] > 0
    known = classes != -1
    assert np.array_equal(written("filled")[known], as_counters(classes)[known])  # the layer wins where it knows something
