"""The information gain through the drop-in C++ headers (tests/cpp/gain_facade_test.cpp): KinematicICP::GridGain on a small grid whose
counters the test sets, against the C entry it wraps and the restatement (tests/gain_ref.py), and the exceptions without a grid and
for a viewpoint outside it."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gain_ref as gr

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "gain_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "gain_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_gain_facade_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_gain_through_the_pipeline(tmp_path):
    occ = gr.random_occupancy(70, 50, 41, unknown=0.25, occupied=0.05)
    occ[20:30, 28:42] = 0  # an open patch round the middle
    views = np.concatenate([np.array([25 * 70 + 35, 22 * 70 + 30, 0, 69, 49 * 70, 50 * 70 - 1], dtype=np.uint32), gr.spread_views(occ, 30, 6)])
    R = 14
    f, prefix = tmp_path / "grid.bin", str(tmp_path / "out")
    with open(f, "wb") as fh:
        np.array([70, 50, R, len(views)], dtype=np.uint32).tofile(fh)
        gr.counts_of(occ).tofile(fh), views.tofile(fh)
    out = subprocess.check_output([build_binary(), str(f), prefix], text=True).splitlines()
    assert "refused_without_grid 1" in out and "refused_outside_the_grid 1" in out and "no_viewpoints 0" in out and "same_as_the_c_entry 1" in out
    want = gr.gain(occ, views, R)
    assert np.array_equal(np.fromfile(prefix + "_rows.bin", dtype=np.uint32).reshape(-1, 4), want)
    assert want[0, 0] > 0 and (want[:, 3] != 0).any() and (want[:, 1] > 0).any() and (want[:, 2] > 0).any()
