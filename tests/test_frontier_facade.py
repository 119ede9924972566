"""The exploration frontiers through the drop-in C++ headers (tests/cpp/frontier_facade_test.cpp): KinematicICP::GridFrontiers on a
small grid whose counters the test sets, against the C entry it wraps and the restatement (tests/frontier_ref.py), and the exceptions
without a grid and without a plan."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import frontier_ref as fr

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "frontier_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "frontier_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_frontier_facade_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_frontiers_through_the_pipeline(tmp_path):
    occ = fr.random_occupancy(70, 50, 41, unknown=0.25, occupied=0.05)
    occ[20:30, 28:42] = 0  # an open patch around the middle cell, the plan's goal
    f, prefix = tmp_path / "grid.bin", str(tmp_path / "out")
    with open(f, "wb") as fh:
        np.array([70, 50], dtype=np.uint32).tofile(fh)
        fr.counts_of(occ).tofile(fh)
    out = subprocess.check_output([build_binary(), str(f), prefix], text=True).splitlines()
    assert "refused_without_grid 1" in out and "refused_without_plan 1" in out and "same_as_the_c_entry 1" in out
    potential = np.fromfile(prefix + "_potential.bin", dtype=np.uint32).reshape(50, 70)
    assert potential[25, 35] == 0
    want_labels = fr.frontiers(occ)[1]
    want = fr.rows_of(want_labels, potential, 2)
    assert "without_plan %d 1" % len(want) in out
    assert np.array_equal(np.fromfile(prefix + "_labels.bin", dtype=np.uint32).reshape(50, 70), want_labels)
    assert np.array_equal(np.fromfile(prefix + "_rows.bin", dtype=np.uint64).reshape(-1, 10), want)
    assert len(want) >= 3 and (want[:, 8] != fr.NONE).any()
