"""The 2-D occupancy grid without a GPU: the walk's properties, a case pinned cell by cell, the two pure-host entries
(K.occupancy_from_counts, K.write_map) against the numpy restatement (tests/grid_ref.py), and grid_host::integrate - the host
restatement of a frame over the very geometry the kernels call (kicp_grid_host.hpp) - in a stand-alone program, built plainly and
under ASan + UBSan, against the restatement on the frames tests/test_gpu_grid.py gives the kernels."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import grid_cases as gc
import grid_ref as gr


def test_walk_properties():
    for a in range(41):
        for b in range(41):
            ox, oy = gr.walk(a, b)
            m = max(a, b)
            assert len(ox) == len(oy) == m  # m cells, the endpoint not among them
            if m == 0:
                continue
            assert (ox[0], oy[0]) == (0, 0)  # the sensor's cell first
            major, minor = (ox, oy) if a >= b else (oy, ox)
            assert np.array_equal(major, np.arange(m))  # exactly one cell per step along the major axis
            assert np.all((np.diff(minor) >= 0) & (np.diff(minor) <= 1))
            assert abs(a - ox[-1]) <= 1 and abs(b - oy[-1]) <= 1 and (ox[-1], oy[-1]) != (a, b)  # ends next to the endpoint
            for sa, sb in ((-1, 1), (1, -1), (-1, -1)):  # mirrored endpoints give mirrored walks
                mx, my = gr.walk(sa * a, sb * b)
                assert np.array_equal(mx, sa * ox) and np.array_equal(my, sb * oy)
            tx, ty = gr.walk(b, a)  # and the transposed endpoint the transposed walk
            assert np.array_equal(tx, oy) and np.array_equal(ty, ox)


def test_pinned_8x6_case_of_the_restatement():
    cfg, points, pose, sensor, hit, miss = gc.pinned_8x6()
    counts = np.zeros((6, 8, 2), dtype=np.uint16)
    assert gr.integrate(cfg, counts, points, pose, sensor) == (2, 0, 2, 11)
    want = np.zeros_like(counts)
    for ix, iy in hit:
        want[iy, ix, 0] = 1
    for ix, iy in miss:
        want[iy, ix, 1] = 1
    assert np.array_equal(counts, want)
    assert gr.integrate(cfg, counts, points[::-1], pose, sensor) == (2, 0, 2, 11)  # the order of the points does not matter
    assert np.array_equal(counts, 2 * want)


PAIRS = [(0, 0), (1, 0), (0, 1), (1, 1), (1, 199), (65535, 65535), (2, 1), (1, 2), (3, 0), (65535, 0), (0, 65535), (7, 3)]


@pytest.mark.parametrize("min_observations", [1, 3])
def test_occupancy_from_counts(min_observations):
    counts = np.array(PAIRS, dtype=np.uint16)
    got = K.occupancy_from_counts(counts, min_observations)
    assert got.dtype == np.int8 and np.array_equal(got, gr.occupancy(counts, min_observations))
    if min_observations == 1:
        assert got[:6].tolist() == [-1, 100, 0, 50, 1, 50]  # (1, 1) and (1, 199) are the rounding ties: halves go up
    else:
        assert got[:6].tolist() == [-1, -1, -1, -1, 1, 50]
    grid = np.arange(24, dtype=np.uint16).reshape(3, 4, 2)
    assert np.array_equal(K.occupancy_from_counts(grid), gr.occupancy(grid))


def test_write_map_bytes(tmp_path):
    # every class of value: unknown, 0, just below / at / above free_thresh, just below / at / above occupied_thresh, 100
    occ = np.array([[-1, 0, 24, 25, 26], [64, 65, 66, 100, -1], [50, 0, 100, -1, 1]], dtype=np.int8)
    prefix = str(tmp_path / "floor")
    K.write_map(prefix, occ, 0.05, -1.5, 2.25)
    pgm, yaml = gr.map_files(prefix, occ, 0.05, -1.5, 2.25)
    got = open(prefix + ".pgm", "rb").read()
    assert got == pgm
    header = b"P5\n5 3\n255\n"
    assert got.startswith(header) and len(got) == len(header) + 15
    assert list(got[len(header):len(header) + 5]) == [205, 254, 0, 205, 254]  # the image's first row is the grid's LAST row
    assert list(got[-5:]) == [205, 254, 254, 205, 205]
    text = open(prefix + ".yaml").read()
    assert text == yaml
    assert text.splitlines() == ["image: floor.pgm", "mode: trinary", "resolution: 0.050000000000000003", "origin: [-1.5, 2.25, 0]", "negate: 0",
                                 "occupied_thresh: 0.65000000000000002", "free_thresh: 0.25"]
    K.write_map(prefix, occ, 0.05, -1.5, 2.25, occupied_thresh=0.5, free_thresh=0.0)  # other thresholds: nothing is free, 50 is not occupied
    assert open(prefix + ".pgm", "rb").read() == gr.map_files(prefix, occ, 0.05, -1.5, 2.25, 0.5, 0.0)[0]


def test_host_entries_argument_errors(tmp_path):
    import ctypes as C
    lib = K.lib()
    occ = np.zeros((2, 2), dtype=np.int8)
    prefix = str(tmp_path / "m")
    for bad in (dict(occupied_thresh=0.25, free_thresh=0.25), dict(occupied_thresh=0.2, free_thresh=0.3), dict(free_thresh=-0.1), dict(occupied_thresh=1.1),
                dict(occupied_thresh=float("nan"))):
        with pytest.raises(K.KicpError) as e:
            K.write_map(prefix, occ, 0.05, 0.0, 0.0, **bad)
        assert e.value.code == K.KICP_ERR_ARG
    for cell, ox in ((0.0, 0.0), (-1.0, 0.0), (float("inf"), 0.0), (0.05, float("nan"))):
        with pytest.raises(K.KicpError) as e:
            K.write_map(prefix, occ, cell, ox, 0.0)
        assert e.value.code == K.KICP_ERR_ARG
    with pytest.raises(K.KicpError) as e:
        K.write_map(prefix, np.zeros((0, 2), dtype=np.int8), 0.05, 0.0, 0.0)
    assert e.value.code == K.KICP_ERR_ARG
    with pytest.raises(K.KicpError) as e:
        K.write_map(str(tmp_path / "no_such_directory" / "m"), occ, 0.05, 0.0, 0.0)
    assert e.value.code == K.KICP_ERR_ARG and "cannot write" in str(e.value)
    ptr = occ.ctypes.data_as(C.POINTER(C.c_byte))
    assert lib.kicp_grid_write_map(None, ptr, 2, 2, 0.05, 0.0, 0.0, 0.65, 0.25) == K.KICP_ERR_ARG
    assert lib.kicp_grid_write_map(prefix.encode(), None, 2, 2, 0.05, 0.0, 0.0, 0.65, 0.25) == K.KICP_ERR_ARG
    counts = np.zeros((4, 2), dtype=np.uint16)
    with pytest.raises(K.KicpError) as e:
        K.occupancy_from_counts(counts, 0)
    assert e.value.code == K.KICP_ERR_ARG
    out = np.zeros(4, dtype=np.int8)
    assert lib.kicp_grid_occupancy_from_counts(None, 4, 1, out.ctypes.data_as(C.POINTER(C.c_byte))) == K.KICP_ERR_ARG
    assert lib.kicp_grid_occupancy_from_counts(counts.ctypes.data_as(C.POINTER(C.c_ushort)), 4, 1, None) == K.KICP_ERR_ARG


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "grid_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.fixture(scope="module")
def host_cases():
    """(cfg, frames, counts after the last frame, stats per frame) per case, by the restatement - computed once"""
    cfg8, points, pose, sensor, _, _ = gc.pinned_8x6()
    cases = [(cfg8, [(points, pose, sensor), (points[:1], pose, sensor), (np.zeros((0, 3)), pose, sensor)]), gc.random_drive()]
    return [(cfg, frames) + tuple(x for x in gc.reference_run(cfg, frames)) for cfg, frames in cases]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_grid_host_integrate_stand_alone(tmp_path, host_cases, flags):
    """grid_host::integrate in a program of its own (tests/cpp/grid_host_test.cpp), as a subprocess; the sanitizers run on this host
    program only"""
    exe = _build(tmp_path, "grid_host_test", flags)
    for k, (cfg, frames, after, stats) in enumerate(host_cases):
        src, dst = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        gc.write_frames(src, cfg, frames)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        got_stats = [tuple(int(v) for v in ln.split()[1:]) for ln in out.stdout.splitlines() if ln.startswith("frame ")]
        assert got_stats == stats
        cells = cfg["width"] * cfg["height"]
        raw = open(dst, "rb").read()
        counts = np.frombuffer(raw[:4 * cells], dtype=np.uint16).reshape(cfg["height"], cfg["width"], 2)
        assert np.array_equal(counts, after[-1])
        assert np.array_equal(np.frombuffer(raw[4 * cells:], dtype=np.int8).reshape(cfg["height"], cfg["width"]), gr.occupancy(after[-1]))
    assert any(s[1] > 0 for s in host_cases[1][3]) and all(s[2] > 0 and s[3] > s[2] for s in host_cases[1][3])  # the drive skips points and carves
