"""The height columns without a GPU: a case of the restatement (tests/elev_ref.py) pinned column by column and class by class, the
pure-host entry (K.traversability_from_columns) against the restatement, and elev_host::integrate / elev_host::classify - the host
restatements over the very arithmetic the kernels call (kicp_elev_host.hpp) - in a stand-alone program, built plainly and under
ASan + UBSan, on the frames and columns tests/test_gpu_elev.py gives the kernels.  Everything is exact: np.array_equal."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import elev_cases as ec
import elev_ref as er


def test_pinned_8x6_case_of_the_restatement():
    cfg, points, pose, sensor, columns, stats, classes = ec.pinned_8x6()
    want = ec.columns_array(cfg, columns)
    got = np.zeros_like(want)
    assert er.integrate(cfg, got, points, pose, sensor) == stats
    for iy in range(cfg["height"]):
        for ix in range(cfg["width"]):
            assert int(got[iy, ix]) == columns.get((ix, iy), 0), (ix, iy)
    again = got.copy()
    assert er.integrate(cfg, again, points[::-1], pose, sensor) == stats[:4] + (0, 0)  # the same frame reversed: nothing is new
    assert np.array_equal(again, got)
    fresh = np.zeros_like(want)
    assert er.integrate(cfg, fresh, points[::-1], pose, sensor) == stats and np.array_equal(fresh, want)  # the order does not matter
    cls, ground, body, step = er.classify(got, 1, 4)
    for iy in range(cfg["height"]):
        for ix in range(cfg["width"]):
            assert cls[iy, ix] == classes.get((ix, iy), -1), (ix, iy)
    assert body[3, 7] and not step[3, 7] and step[1, 4] and not body[1, 4] and not step[1, 3]  # the HIGHER cell of the edge is marked
    assert (ground[3, 7], ground[5, 2], ground[1, 3], ground[1, 4], ground[0, 0]) == (2, 3, 0, 62, 255)
    assert er.counts(cls, body) == (44, 2, 1, 1)
    got_cls, got_ground, got_counts = K.traversability_from_columns(got, 1, 4, return_ground=True, return_counts=True)
    assert np.array_equal(got_cls, cls) and np.array_equal(got_ground, ground) and got_counts == (44, 2, 1, 1)


def check_host_entry(columns):
    for S, H in ec.PARAMS:
        cls, ground, body, _ = er.classify(columns, S, H)
        for rect in ec.RECTS:
            r = rect or (0, 0, ec.W70, ec.H45)
            got, got_ground, got_counts = K.traversability_from_columns(columns, S, H, rect=rect, return_ground=True, return_counts=True)
            assert got.dtype == np.int8 and got_ground.dtype == np.uint8 and got.shape == (r[3], r[2])
            assert np.array_equal(got, er.restrict(cls, r)) and np.array_equal(got_ground, er.restrict(ground, r)), (S, H, rect)
            assert got_counts == er.counts(er.restrict(cls, r), er.restrict(body, r)), (S, H, rect)
        assert np.array_equal(K.traversability_from_columns(columns, S, H), cls)  # the classes alone


@pytest.mark.parametrize("kind", ["dense", "sparse", "zero"])
def test_traversability_from_random_columns(kind):
    check_host_entry(ec.random_columns(kind))


def test_traversability_from_handmade_columns():
    columns = ec.handmade_columns()
    check_host_entry(columns)
    # the places a shift by 64 would get wrong, spelled out
    top = K.traversability_from_columns(columns, 0, 64)
    assert top[8, 2] == 0 and top[8, 5] == 100 and top[8, 11] == 100  # only bit 63: nothing above it; ground 60 and bit 63; a full column
    widest = K.traversability_from_columns(columns, 62, 63)
    assert widest[8, 14] == 100 and widest[8, 17] == 0 and widest[8, 20] == 0 and widest[8, 11] == 100
    least = K.traversability_from_columns(columns, 0, 1)
    assert least[5, 3] == 100 and least[5, 2] == 0 and least[8, 8] == 100 and least[8, 5] == 0  # bit 61 is BODY over 60 at H = 1, bit 63 is overhead
    step = K.traversability_from_columns(columns, 2, 8)
    for x, y in ((15, 20), (31, 20), (47, 20), (63, 20)):
        assert (step[y, x], step[y, x + 1], step[y + 2, x], step[y + 2, x + 1]) == (0, 100, 100, 0)
    assert step[16, 32] == 100 and step[15, 31] == 0 and step[15, 48] == 100 and step[16, 47] == 0
    assert step[0, 0] == 100 and step[1, 1] == 0 and step[ec.H45 - 1, ec.W70 - 1] == 100 and step[30, 60] == 0 and step[36, 1] == 100 and step[36, 0] == 0


def test_host_entry_argument_errors():
    import ctypes as C
    columns = np.zeros((4, 5), dtype=np.uint64)
    for S, H in ((63, 64), (0, 0), (3, 3), (4, 2), (0, 65)):
        with pytest.raises(K.KicpError) as e:
            K.traversability_from_columns(columns, S, H)
        assert e.value.code == K.KICP_ERR_ARG, (S, H)
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (5, 0, 1, 1), (0, 4, 1, 1), (3, 0, 3, 1), (0, 2, 1, 3)):
        with pytest.raises(K.KicpError) as e:
            K.traversability_from_columns(columns, 1, 4, rect=rect)
        assert e.value.code == K.KICP_ERR_ARG, rect
    with pytest.raises(K.KicpError) as e:
        K.traversability_from_columns(np.zeros(5, dtype=np.uint64), 1, 4)
    assert e.value.code == K.KICP_ERR_ARG
    lib, cfg = K.lib(), K.ElevationTraversabilityConfig(1, 4)
    out = np.zeros(20, dtype=np.int8)
    cp, op = columns.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.ctypes.data_as(C.POINTER(C.c_byte))
    assert lib.kicp_elev_traversability_from_columns(None, 5, 4, C.byref(cfg), 0, 0, 5, 4, op, None, None, 20) == K.KICP_ERR_ARG
    assert lib.kicp_elev_traversability_from_columns(cp, 5, 4, None, 0, 0, 5, 4, op, None, None, 20) == K.KICP_ERR_ARG
    assert lib.kicp_elev_traversability_from_columns(cp, 5, 4, C.byref(cfg), 0, 0, 5, 4, None, None, None, 20) == K.KICP_ERR_ARG
    assert lib.kicp_elev_traversability_from_columns(cp, 5, 4, C.byref(cfg), 0, 0, 5, 4, op, None, None, 19) == K.KICP_ERR_ARG
    assert lib.kicp_elev_traversability_from_columns(cp, 0, 4, C.byref(cfg), 0, 0, 5, 4, op, None, None, 20) == K.KICP_ERR_ARG
    assert lib.kicp_elev_traversability_from_columns(cp, 16385, 16384, C.byref(cfg), 0, 0, 5, 4, op, None, None, 20) == K.KICP_ERR_CAPACITY
    assert "2^28" in lib.kicp_last_error().decode()
    assert lib.kicp_elev_traversability_from_columns(cp, 5, 4, C.byref(cfg), 0, 0, 5, 4, op, None, None, 20) == K.KICP_OK and (out == -1).all()


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "elev_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.fixture(scope="module")
def host_cases():
    """(cfg, frames, starting columns or None, columns after the last frame, stats per frame) per case, by the restatement - once"""
    cfg8, points, pose, sensor, _, _, _ = ec.pinned_8x6()
    one = [(np.array([p], dtype=np.float64), ec.IDENTITY, ec.SENSOR16) for p, _, _ in ec.ONE_POINT.values()]
    nan_pose = np.array([0.0, 0.0, 0.0, 1.0, np.nan, 0.0, 0.0])
    contended = [(ec.contended_three(), ec.IDENTITY, ec.SENSOR16)] * 2 + [(ec.contended_one_cell(), ec.IDENTITY, ec.SENSOR16), ec.tilted_frame(),
                                                                         (ec.INSIDE_REACH_OUTSIDE_GRID, ec.IDENTITY, ec.SENSOR16_EAST),
                                                                         (ec.contended_three(), nan_pose, ec.SENSOR16),
                                                                         (ec.contended_three(), ec.IDENTITY, np.array([np.nan, 0.0, 0.0]))]
    cases = [(cfg8, [(points, pose, sensor), (points[:1], pose, sensor), (np.zeros((0, 3)), pose, sensor)], None), (ec.CFG16, one + contended, None),
             ec.random_drive() + (None,)]
    out = [(cfg, frames, start) + tuple(ec.reference_run(cfg, frames)) for cfg, frames, start in cases]
    # frames: none; the columns the classification can get wrong, as the layer's starting point
    cfg70 = er.make_config(0.25, 0.0, 0.0, ec.W70, ec.H45, 0.0, 0.125, 2.0)
    for columns in (ec.handmade_columns(), ec.random_columns("dense"), ec.random_columns("sparse")):
        out.append((cfg70, [], columns, [columns], []))
    return out


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_elev_host_stand_alone(tmp_path, host_cases, flags):
    """elev_host::integrate and elev_host::classify in a program of its own (tests/cpp/elev_host_test.cpp), as a subprocess; the
    sanitizers run on this host program only"""
    exe = _build(tmp_path, "elev_host_test", flags)
    for k, (cfg, frames, start, after, stats) in enumerate(host_cases):
        src, dst, begin = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k)), str(tmp_path / ("start%d.bin" % k))
        ec.write_frames(src, cfg, frames, ec.PARAMS)
        if start is not None:
            start.tofile(begin)
        out = subprocess.run([exe, src, dst] + ([begin] if start is not None else []), capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        lines = out.stdout.splitlines()
        assert [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("frame ")] == stats
        cells, shape = cfg["width"] * cfg["height"], (cfg["height"], cfg["width"])
        raw = open(dst, "rb").read()
        assert len(raw) == cells * (8 + 2 * len(ec.PARAMS))
        columns = np.frombuffer(raw[:8 * cells], dtype=np.uint64).reshape(shape)
        assert np.array_equal(columns, after[-1])
        got_counts = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("counts ")]
        for j, (S, H) in enumerate(ec.PARAMS):
            cls, ground, body, _ = er.classify(after[-1], S, H)
            at = 8 * cells + 2 * j * cells
            assert np.array_equal(np.frombuffer(raw[at:at + cells], dtype=np.int8).reshape(shape), cls), (k, S, H)
            assert np.array_equal(np.frombuffer(raw[at + cells:at + 2 * cells], dtype=np.uint8).reshape(shape), ground), (k, S, H)
            assert got_counts[j] == er.counts(cls, body)
    # what the cases are there for: every class of point, contended pairs, and a drive that fills columns
    s16 = host_cases[1][4]
    n_one = len(ec.ONE_POINT)
    assert [s[:4] for s in s16[:n_one]] == [tuple(int(c == k) for k in (er.USED, er.SKIPPED, er.OUTSIDE_GRID, er.OUTSIDE_COLUMN)) for _, c, _ in ec.ONE_POINT.values()]
    assert s16[n_one] == (4096, 0, 0, 0, 3, 3) and s16[n_one + 1] == (4096, 0, 0, 0, 0, 0) and s16[n_one + 2][4:] == (64, 1)
    assert s16[n_one + 4] == (0, 0, 1, 0, 0, 0) and s16[n_one + 5] == s16[n_one + 6] == (0, 4096, 0, 0, 0, 0)
    drive = host_cases[2][4]
    assert all(s[0] > 1000 and s[1] > 0 and s[4] > 500 and s[5] > 100 for s in drive) and any(s[2] > 0 for s in drive) and any(s[3] > 0 for s in drive)
