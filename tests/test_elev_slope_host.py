"""The slope limit of the height columns without a GPU: the pure-host entry (K.traversability_slope_from_columns) against the
restatement (tests/elev_slope_ref.py) on every case of tests/elev_slope_cases.py; elev_host::classify_slope - the host restatement over
the very arithmetic the kernels call (kicp_elev_host.hpp) - in a stand-alone program, built plainly and under ASan + UBSan, on the
same cases; the ramp scene that says what the limit is for; kicp_elev_slope_limit; and the argument errors.  Everything is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import elev_ref as er
import elev_slope_cases as sc
import elev_slope_ref as sr


def drive_case():
    return ("drive", sc.drive_columns()[2], sc.DRIVE_PARAMS, sc.DRIVE_SLOPE, [None, (100, 120, 77, 45)])


@pytest.mark.parametrize("which", ["small", "random", "drive"])
def test_host_entry_against_the_restatement(which):
    for case in {"small": sc.small_cases, "random": sc.random_cases, "drive": lambda: [drive_case()]}[which]():
        name, columns, (S, H), slope, rects = case
        for rect in rects:
            got, ground, fit, counts = K.traversability_slope_from_columns(columns, S, H, slope, rect=rect, return_ground=True, return_fit=True, return_counts=True)
            sc.check_result(case, rect, got, ground, fit, counts)
        sc.check_result(case, None, K.traversability_slope_from_columns(columns, S, H, slope))  # the classes alone
        got, fit = K.traversability_slope_from_columns(columns, S, H, K.ElevationSlopeConfig(*slope), return_fit=True)
        sc.check_result(case, None, got, got_fit=fit)
        # wherever a cell is not SLOPE only, its value is kicp_elev_traversability's
        want = sc.expected(case)
        only = want.slope & ~want.body & ~want.step
        plain = K.traversability_from_columns(columns, S, H)
        assert np.array_equal(got[~only], plain[~only]) and (got[only] == 100).all() and (plain[only] == 0).all(), name


@pytest.mark.parametrize("case", sc.radius_cases(), ids=lambda case: case[0])
def test_host_entry_at_every_radius(case):
    name, columns, (S, H), slope, rects = case
    assert (sc.expected(case).fit[:, :, 0] > 0).any(), name  # some cell has a fit
    for rect in rects:
        got, ground, fit, counts = K.traversability_slope_from_columns(columns, S, H, slope, rect=rect, return_ground=True, return_fit=True, return_counts=True)
        sc.check_result(case, rect, got, ground, fit, counts)


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "elev_slope_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_elev_slope_host_stand_alone(tmp_path, flags):
    """elev_host::classify_slope in a program of its own (tests/cpp/elev_slope_host_test.cpp), as a subprocess; the sanitizers run on
    this host program only"""
    exe = _build(tmp_path, "elev_slope_host_test", flags)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for case in sc.all_cases() + [drive_case()]:
        name, columns, (S, H), slope, rects = case
        height, width = columns.shape
        full = [rect or (0, 0, width, height) for rect in rects]
        with open(src, "wb") as f:
            np.array([width, height, len(full)], dtype=np.float64).tofile(f)
            np.array([[S, H] + list(slope) + list(r) for r in full], dtype=np.float64).tofile(f)
            np.ascontiguousarray(columns, dtype=np.uint64).tofile(f)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (name, (out.stdout + out.stderr)[-2000:])
        got_counts = [tuple(int(v) for v in ln.split()[1:]) for ln in out.stdout.splitlines() if ln.startswith("counts ")]
        raw, at = open(dst, "rb").read(), 0
        for k, r in enumerate(full):
            n = r[2] * r[3]
            classes = np.frombuffer(raw[at:at + n], dtype=np.int8).reshape(r[3], r[2])
            ground = np.frombuffer(raw[at + n:at + 2 * n], dtype=np.uint8).reshape(r[3], r[2])
            fit = np.frombuffer(raw[at + 2 * n:at + 26 * n], dtype=np.int64).reshape(r[3], r[2], 3)
            at += 26 * n
            sc.check_result(case, r, classes, ground, fit, got_counts[k])
        assert at == len(raw) and len(got_counts) == len(full)


# ---- what the limit is for: planes of 0 .. 35 degrees, seen as a 3-D lidar sees ground ----------------------------------------------
RAMP_CELL, RAMP_SLAB, RAMP_SIDE, RAMP_SEED = 0.1, 0.0625, 40, 3


def ramp_columns(degrees, rng):
    """a plane of that inclination in a random direction on RAMP_SIDE^2 cells, 1 cm of height noise per cell, 30 % of the cells known"""
    direction = rng.uniform(0.0, 2.0 * np.pi)
    y, x = np.mgrid[0:RAMP_SIDE, 0:RAMP_SIDE]
    z = np.tan(np.deg2rad(degrees)) * RAMP_CELL * (np.cos(direction) * x + np.sin(direction) * y) + rng.normal(0.0, 0.01, (RAMP_SIDE, RAMP_SIDE))
    g = np.floor((z - z.min() + 0.2) / RAMP_SLAB).astype(np.int64)
    assert g.min() >= 0 and g.max() <= 63
    g[rng.random((RAMP_SIDE, RAMP_SIDE)) >= 0.3] = 255
    return sc.from_grounds(g)


def test_a_20_degree_limit_tells_ramps_apart_where_step_sees_nothing():
    rise, run = K.elev_slope_limit(RAMP_CELL, RAMP_SLAB, np.tan(np.deg2rad(20.0)))
    assert (rise, run) == sr.slope_limit(RAMP_CELL, RAMP_SLAB, np.tan(np.deg2rad(20.0))) == (596, 1024)
    slope = (4, 6, 12, rise, run)
    rng = np.random.default_rng(RAMP_SEED)
    for degrees in (0, 10, 15, 25, 35):
        columns = ramp_columns(degrees, rng)
        got, fit, counts = K.traversability_slope_from_columns(columns, 2, 24, slope, return_fit=True, return_counts=True)
        want = sr.classify(columns, 2, 24, slope)
        assert np.array_equal(got, want.classes) and np.array_equal(fit, want.fit) and counts == sr.counts(want)
        known, fitted = columns != 0, fit[:, :, 0] > 0
        print("%d degrees: %d known cells, %d with a fit, counts %s" % (degrees, known.sum(), fitted.sum(), counts))
        assert 350 < known.sum() < 620 and fitted.sum() > 100
        plain = K.traversability_from_columns(columns, 2, 24)
        assert (plain[known] == 0).all() and counts[2] == counts[3] == 0  # the gap: BODY and STEP call every known cell of every plane traversable
        if degrees <= 15:
            assert counts[4] == 0 and (got[known] == 0).all()
        else:
            assert (got[fitted] == 100).all() and counts[4] == fitted.sum() and (got[known & ~fitted] == 0).all()


def test_slope_limit():
    for cell, slab, tangent in ((0.1, 0.0625, 0.36397), (0.05, 0.125, 1.0), (0.25, 0.125, 0.0), (0.1, 0.0625, 39.99), (1.0, 1.0, 63.999), (0.3, 0.7, 0.57735)):
        assert K.elev_slope_limit(cell, slab, tangent) == sr.slope_limit(cell, slab, tangent) != None  # noqa: E711
    assert K.elev_slope_limit(1.0, 1.0, 65535.0 / 1024.0) == (65535, 1024) and K.elev_slope_limit(0.1, 0.0625, -0.0) == (0, 1024)
    for cell, slab, tangent in ((1.0, 1.0, 64.0), (0.1, 0.0625, -1e-9), (0.1, 0.0625, np.nan), (0.1, 0.0625, np.inf), (0.1, 0.0625, -np.inf), (0.0, 0.0625, 0.3),
                                (0.1, 0.0, 0.3), (np.nan, 0.0625, 0.3), (0.1, np.inf, 0.3), (-0.1, 0.0625, 0.3)):
        assert sr.slope_limit(cell, slab, tangent) is None or not (cell > 0 and np.isfinite(cell) and slab > 0 and np.isfinite(slab))
        with pytest.raises(K.KicpError) as e:
            K.elev_slope_limit(cell, slab, tangent)
        assert e.value.code == K.KICP_ERR_ARG, (cell, slab, tangent)
    lib, cfg, rise, run = K.lib(), K.ElevationConfig(0.1, 0, 0, 4, 4, 0.0, 0.0625, 1.0), C.c_uint(7), C.c_uint(7)
    assert lib.kicp_elev_slope_limit(None, 0.3, C.byref(rise), C.byref(run)) == K.KICP_ERR_ARG
    assert lib.kicp_elev_slope_limit(C.byref(cfg), 0.3, None, C.byref(run)) == K.KICP_ERR_ARG
    assert lib.kicp_elev_slope_limit(C.byref(cfg), 0.3, C.byref(rise), None) == K.KICP_ERR_ARG and (rise.value, run.value) == (7, 7)
    assert lib.kicp_elev_slope_limit(C.byref(cfg), 0.3, C.byref(rise), C.byref(run)) == K.KICP_OK and (rise.value, run.value) == sr.slope_limit(0.1, 0.0625, 0.3)


GOOD = (4, 6, 12, 596, 1024)
BAD_SLOPES = [(0, 6, 12, 1, 1), (9, 6, 12, 1, 1), (4, 64, 12, 1, 1), (4, 6, 2, 1, 1), (4, 6, 290, 1, 1), (4, 6, 12, 65536, 1), (4, 6, 12, 1, 0), (4, 6, 12, 1, 65536),
              (2 ** 32 - 1, 6, 12, 1, 1)]
EDGE_SLOPES = [(1, 0, 3, 0, 1), (8, 63, 289, 65535, 65535)]


def test_host_entry_argument_errors():
    columns = np.zeros((4, 5), dtype=np.uint64)
    for slope in BAD_SLOPES:
        with pytest.raises(K.KicpError) as e:
            K.traversability_slope_from_columns(columns, 1, 4, slope)
        assert e.value.code == K.KICP_ERR_ARG, slope
    for slope in EDGE_SLOPES:
        assert (K.traversability_slope_from_columns(columns, 1, 4, slope) == -1).all()
    for S, H in ((63, 64), (0, 0), (3, 3), (4, 2), (0, 65)):  # the traversability configuration is checked as ever
        with pytest.raises(K.KicpError) as e:
            K.traversability_slope_from_columns(columns, S, H, GOOD)
        assert e.value.code == K.KICP_ERR_ARG, (S, H)
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (5, 0, 1, 1), (0, 4, 1, 1), (3, 0, 3, 1), (0, 2, 1, 3)):
        with pytest.raises(K.KicpError) as e:
            K.traversability_slope_from_columns(columns, 1, 4, GOOD, rect=rect)
        assert e.value.code == K.KICP_ERR_ARG, rect
    with pytest.raises(K.KicpError) as e:
        K.traversability_slope_from_columns(np.zeros(5, dtype=np.uint64), 1, 4, GOOD)
    assert e.value.code == K.KICP_ERR_ARG
    lib, cfg, slope = K.lib(), K.ElevationTraversabilityConfig(1, 4), K.ElevationSlopeConfig(*GOOD)
    out = np.zeros(20, dtype=np.int8)
    cp, op = columns.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.ctypes.data_as(C.POINTER(C.c_byte))
    call = lib.kicp_elev_traversability_slope_from_columns
    assert call(None, 5, 4, C.byref(cfg), C.byref(slope), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, None, C.byref(slope), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, C.byref(cfg), None, 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, C.byref(cfg), C.byref(slope), 0, 0, 5, 4, None, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, C.byref(cfg), C.byref(slope), 0, 0, 5, 4, op, None, None, None, 19) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, C.byref(cfg), C.byref(slope), 0, 0, 5, 4, op, None, None, None, 21) == K.KICP_ERR_ARG
    assert call(cp, 0, 4, C.byref(cfg), C.byref(slope), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 16385, 16384, C.byref(cfg), C.byref(slope), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_CAPACITY
    assert call(cp, 5, 4, C.byref(cfg), C.byref(slope), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_OK and (out == -1).all()
