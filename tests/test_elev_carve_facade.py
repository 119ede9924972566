"""The height columns' carve through the drop-in C++ headers (tests/cpp/elev_carve_facade_test.cpp): the six-frame drive of
tests/test_elev_facade.py through KinematicICP with a layer, carving off - the default - and on.  Poses and returned clouds must be
bit-equal between the two runs; with carving off the columns and the six words must be plain integration's; with carving on the
columns and the nine words must be the restatement's update (tests/elev_carve_ref.py) of the returned frames at the returned poses; a
copy made after frame 3, moved and assigned, must carry the setting and end with the same layer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import elev_carve_ref as ecr
import elev_ref as er
import test_elev_facade as tef

BIN = os.path.join(ROOT, "tests", "cpp", "elev_carve_facade_test")
CARVE = (2, 1, 1)


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "elev_carve_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(tef.CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", tef.CPP, "-I", os.path.join(tef.CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_elev_carve_facade_compiles_and_links():
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_carving_through_the_pipeline(tmp_path):
    f, g, prefix = tmp_path / "pipe.bin", tmp_path / "layer.bin", str(tmp_path / "out")
    ext = tef.write_drive(f)
    cfg = er.make_config(0.1, -14.0, -14.0, 300, 300, -1.0, 0.0625, 12.0)
    np.array([cfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_origin", "slab", "max_ray")] + list(CARVE), dtype=np.float64).tofile(g)
    out = subprocess.check_output([build_binary(), str(f), str(g), prefix], text=True).splitlines()
    for line in ("refused_without_layer 1", "off_by_default 1", "refused_bad_config 1", "off_carve_stats_stay_zero 1", "copy_carves 1", "moved_carves 1", "assigned_carves 1",
                 "six_words_agree 1", "copy_stats_agree 1", "disabled 1", "new_layer_starts_off 1"):
        assert line in out, line

    # poses and returned clouds: bit-equal with carving off and on
    assert open(prefix + "_off.bin", "rb").read() == open(prefix + "_on.bin", "rb").read()
    run = tef._read_run(prefix + "_on.bin", 6)
    plain, carved = np.zeros((300, 300), dtype=np.uint64), np.zeros((300, 300), dtype=np.uint64)
    off = [tuple(int(v) for v in ln.split()[2:]) for ln in out if ln.startswith("off ")]
    on = [tuple(int(v) for v in ln.split()[2:]) for ln in out if ln.startswith("on ")]
    for k, (pose, frame, _) in enumerate(run):
        assert er.integrate(cfg, plain, frame, pose, ext[4:]) == off[k]  # carving off: today's statistics
        want = ecr.update(cfg, carved, frame, pose, ext[4:], *CARVE)
        print("frame %d: restatement %s, pipeline %s" % (k, want, on[k]))
        assert want == on[k] and want[6] > 1000 and (k == 0 or want[7] > 0) and want[8] == 0
    assert np.array_equal(np.fromfile(prefix + "_off_columns.bin", dtype=np.uint64).reshape(300, 300), plain)  # ... and today's columns
    assert np.array_equal(np.fromfile(prefix + "_on_columns.bin", dtype=np.uint64).reshape(300, 300), carved)
    assert np.array_equal(np.fromfile(prefix + "_copy_columns.bin", dtype=np.uint64).reshape(300, 300), carved)
    assert not np.array_equal(plain, carved)
