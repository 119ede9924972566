"""The class ROUGH of the height columns without a GPU: the pure-host entry (K.traversability_rough_from_columns) against the
restatement (tests/elev_rough_ref.py) on every case of tests/elev_rough_cases.py; elev_host::classify_rough - the host restatement
over the very arithmetic the kernels call (kicp_elev_host.hpp) - in a stand-alone program, built plainly and under ASan + UBSan, on
the same cases; the planes and the rubble field that say what the class is for; kicp_elev_rough_limit; and the argument errors.
Everything is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import elev_rough_cases as rc
import elev_rough_ref as rr
import elev_slope_cases as sc
import elev_slope_ref as sr
from test_elev_slope_host import RAMP_CELL, RAMP_SIDE, RAMP_SLAB, ramp_columns


def drive_case():
    return ("drive", sc.drive_columns()[2], sc.DRIVE_PARAMS, sc.DRIVE_SLOPE, rc.DRIVE_ROUGH, [None, (100, 120, 77, 45)])


@pytest.mark.parametrize("which", ["small", "random", "drive"])
def test_host_entry_against_the_restatement(which):
    for case in {"small": rc.small_cases, "random": rc.random_cases, "drive": lambda: [drive_case()]}[which]():
        name, columns, (S, H), slope, rough, rects = case
        for rect in rects:
            got, ground, fit, counts = K.traversability_rough_from_columns(columns, S, H, slope, rough, rect=rect, return_ground=True, return_fit=True, return_counts=True)
            rc.check_result(case, rect, got, ground, fit, counts)
        rc.check_result(case, None, K.traversability_rough_from_columns(columns, S, H, slope, rough))  # the classes alone
        got, fit = K.traversability_rough_from_columns(columns, S, H, K.ElevationSlopeConfig(*slope), K.ElevationRoughConfig(*rough), return_fit=True)
        rc.check_result(case, None, got, got_fit=fit)
        # wherever a cell is not ROUGH only, its value is kicp_elev_traversability_slope's, and the fit begins with its triple
        want = rc.expected(case)
        only = want.rough & ~want.body & ~want.step & ~want.slope
        plain, triple = K.traversability_slope_from_columns(columns, S, H, slope, return_fit=True)
        assert np.array_equal(got[~only], plain[~only]) and (got[only] == 100).all() and (plain[only] == 0).all(), name
        assert np.array_equal(fit[:, :, :3], triple), name


@pytest.mark.parametrize("case", rc.radius_cases(), ids=lambda case: case[0])
def test_host_entry_at_every_radius(case):
    name, columns, (S, H), slope, rough, rects = case
    assert (rc.expected(case).fit[:, :, 0] > 0).any(), name  # some cell has a fit
    for rect in rects:
        got, ground, fit, counts = K.traversability_rough_from_columns(columns, S, H, slope, rough, rect=rect, return_ground=True, return_fit=True, return_counts=True)
        rc.check_result(case, rect, got, ground, fit, counts)


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "elev_rough_host_test.cpp"), "-o", exe] + extra)
    return exe


BUILDS = pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])


@BUILDS
def test_elev_rough_host_stand_alone(tmp_path, flags):
    """elev_host::classify_rough in a program of its own (tests/cpp/elev_rough_host_test.cpp), as a subprocess; the sanitizers run on
    this host program only"""
    exe = _build(tmp_path, "elev_rough_host_test", flags)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for case in rc.all_cases() + [drive_case()]:
        name, columns, (S, H), slope, rough, rects = case
        height, width = columns.shape
        full = [rect or (0, 0, width, height) for rect in rects]
        with open(src, "wb") as f:
            np.array([width, height, len(full)], dtype=np.float64).tofile(f)
            np.array([[S, H] + list(slope) + list(rough) + list(r) for r in full], dtype=np.float64).tofile(f)
            np.ascontiguousarray(columns, dtype=np.uint64).tofile(f)
        out = subprocess.run([exe, "rough", src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (name, (out.stdout + out.stderr)[-2000:])
        got_counts = [tuple(int(v) for v in ln.split()[1:]) for ln in out.stdout.splitlines() if ln.startswith("counts ")]
        raw, at = open(dst, "rb").read(), 0
        for k, r in enumerate(full):
            n = r[2] * r[3]
            classes = np.frombuffer(raw[at:at + n], dtype=np.int8).reshape(r[3], r[2])
            ground = np.frombuffer(raw[at + n:at + 2 * n], dtype=np.uint8).reshape(r[3], r[2])
            fit = np.frombuffer(raw[at + 2 * n:at + 42 * n], dtype=np.int64).reshape(r[3], r[2], 5)
            at += 42 * n
            rc.check_result(case, r, classes, ground, fit, got_counts[k])
        assert at == len(raw) and len(got_counts) == len(full)


# ---- what the class is for: planes that are not ROUGH, and rubble that STEP and SLOPE call traversable ------------------------------
ROUGH_LIMIT, ROUGH_SLOPE, ROUGH_SEED, RUBBLE_AMPLITUDE = (1, 2), (4, 6, 12, 596, 1024), 3, 0.10  # half a slab^2; the slope suite's limit; +- 10 cm


def rubble_columns(rng):
    """RAMP_SIDE^2 cells of RAMP_CELL, 30 % known, the grounds uniform in +- RUBBLE_AMPLITUDE around a level plane 0.2 m over z_origin"""
    z = rng.uniform(-RUBBLE_AMPLITUDE, RUBBLE_AMPLITUDE, (RAMP_SIDE, RAMP_SIDE))
    g = np.floor((z + 0.2) / RAMP_SLAB).astype(np.int64)
    g[rng.random((RAMP_SIDE, RAMP_SIDE)) >= 0.3] = 255
    return sc.from_grounds(g)


def mean_squared_residual(fit):
    fitted = fit[:, :, 0] > 0
    return fit[:, :, 3][fitted] / (fit[:, :, 4][fitted] * fit[:, :, 0][fitted])


def test_planes_are_not_rough_and_rubble_is_where_step_and_slope_see_nothing():
    assert (RAMP_CELL, RAMP_SLAB, RAMP_SIDE) == (0.1, 0.0625, 40)
    rng = np.random.default_rng(ROUGH_SEED)
    for degrees in (0, 5, 10, 15):
        columns = ramp_columns(degrees, rng)
        got, fit, counts = K.traversability_rough_from_columns(columns, 3, 24, ROUGH_SLOPE, ROUGH_LIMIT, return_fit=True, return_counts=True)
        want = rr.classify(columns, 3, 24, ROUGH_SLOPE, ROUGH_LIMIT)
        assert np.array_equal(got, want.classes) and np.array_equal(fit, want.fit) and counts == rr.counts(want)
        fitted = fit[:, :, 0] > 0
        print("%d degrees: %d known cells, %d with a fit, counts %s, the worst mean squared residual %.3f slab^2" %
              (degrees, (columns != 0).sum(), fitted.sum(), counts, mean_squared_residual(fit).max()))
        assert fitted.sum() > 100 and not want.rough.any() and counts[5] == 0 and (got[columns != 0] == 0).all()
    columns = rubble_columns(rng)
    known = columns != 0
    slope_says = K.traversability_slope_from_columns(columns, 3, 24, ROUGH_SLOPE)
    assert np.array_equal(slope_says, sr.classify(columns, 3, 24, ROUGH_SLOPE).classes) and (slope_says[known] == 0).all()  # the gap
    got, fit, counts = K.traversability_rough_from_columns(columns, 3, 24, ROUGH_SLOPE, ROUGH_LIMIT, return_fit=True, return_counts=True)
    want = rr.classify(columns, 3, 24, ROUGH_SLOPE, ROUGH_LIMIT)
    assert np.array_equal(got, want.classes) and np.array_equal(fit, want.fit) and counts == rr.counts(want)
    fitted = fit[:, :, 0] > 0
    print("rubble: %d known cells, %d with a fit, counts %s, %d of the fitted cells ROUGH, the median mean squared residual %.3f slab^2" %
          (known.sum(), fitted.sum(), counts, want.rough.sum(), np.median(mean_squared_residual(fit))))
    assert 350 < known.sum() < 620 and fitted.sum() > 100 and counts[2] == counts[3] == counts[4] == 0
    assert 10 * want.rough.sum() >= 9 * fitted.sum() and counts[5] == want.rough.sum() and (got[want.rough] == 100).all()


def test_rough_limit():
    for slab, rms in ((0.0625, 0.0442), (0.125, 0.125), (0.125, 0.0), (0.0625, 0.49), (1.0, 7.99), (0.7, 0.3)):
        assert K.elev_rough_limit(slab, rms) == rr.rough_limit(slab, rms) != None  # noqa: E711
    assert K.elev_rough_limit(1.0, 1.0) == (1024, 1024) and K.elev_rough_limit(0.0625, -0.0) == (0, 1024) and K.elev_rough_limit(0.0625, -0.0625) == (1024, 1024)
    assert K.elev_rough_limit(1.0, np.sqrt(65535.0 / 1024.0)) == rr.rough_limit(1.0, np.sqrt(65535.0 / 1024.0))
    for slab, rms in ((1.0, 8.0), (0.0625, np.nan), (0.0625, np.inf), (0.0625, -np.inf), (0.0, 0.3), (np.nan, 0.3), (np.inf, 0.3), (-0.1, 0.3)):
        assert rr.rough_limit(slab, rms) is None or not (slab > 0 and np.isfinite(slab))
        with pytest.raises(K.KicpError) as e:
            K.elev_rough_limit(slab, rms)
        assert e.value.code == K.KICP_ERR_ARG, (slab, rms)
    lib, cfg, num, den = K.lib(), K.ElevationConfig(0.1, 0, 0, 4, 4, 0.0, 0.0625, 1.0), C.c_uint(7), C.c_uint(7)
    assert lib.kicp_elev_rough_limit(None, 0.03, C.byref(num), C.byref(den)) == K.KICP_ERR_ARG
    assert lib.kicp_elev_rough_limit(C.byref(cfg), 0.03, None, C.byref(den)) == K.KICP_ERR_ARG
    assert lib.kicp_elev_rough_limit(C.byref(cfg), 0.03, C.byref(num), None) == K.KICP_ERR_ARG and (num.value, den.value) == (7, 7)
    assert lib.kicp_elev_rough_limit(C.byref(cfg), 0.03, C.byref(num), C.byref(den)) == K.KICP_OK and (num.value, den.value) == rr.rough_limit(0.0625, 0.03)


GOOD, GOOD_ROUGH = (4, 6, 12, 596, 1024), (1, 2)
BAD_ROUGH = [(65536, 1), (0, 0), (1, 65536), (2 ** 32 - 1, 1), (1, 2 ** 32 - 1)]
EDGE_ROUGH = [(0, 1), (65535, 65535), (0, 65535), (65535, 1)]


def test_host_entry_argument_errors():
    from test_elev_slope_host import BAD_SLOPES
    columns = np.zeros((4, 5), dtype=np.uint64)
    for rough in BAD_ROUGH:
        with pytest.raises(K.KicpError) as e:
            K.traversability_rough_from_columns(columns, 1, 4, GOOD, rough)
        assert e.value.code == K.KICP_ERR_ARG, rough
    for rough in EDGE_ROUGH:
        assert (K.traversability_rough_from_columns(columns, 1, 4, GOOD, rough) == -1).all()
    for slope in BAD_SLOPES:
        with pytest.raises(K.KicpError) as e:
            K.traversability_rough_from_columns(columns, 1, 4, slope, GOOD_ROUGH)
        assert e.value.code == K.KICP_ERR_ARG, slope
    for S, H in ((63, 64), (0, 0), (3, 3), (4, 2), (0, 65)):
        with pytest.raises(K.KicpError) as e:
            K.traversability_rough_from_columns(columns, S, H, GOOD, GOOD_ROUGH)
        assert e.value.code == K.KICP_ERR_ARG, (S, H)
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (5, 0, 1, 1), (0, 4, 1, 1), (3, 0, 3, 1), (0, 2, 1, 3)):
        with pytest.raises(K.KicpError) as e:
            K.traversability_rough_from_columns(columns, 1, 4, GOOD, GOOD_ROUGH, rect=rect)
        assert e.value.code == K.KICP_ERR_ARG, rect
    with pytest.raises(K.KicpError) as e:
        K.traversability_rough_from_columns(np.zeros(5, dtype=np.uint64), 1, 4, GOOD, GOOD_ROUGH)
    assert e.value.code == K.KICP_ERR_ARG
    lib, cfg, slope, rough = K.lib(), K.ElevationTraversabilityConfig(1, 4), K.ElevationSlopeConfig(*GOOD), K.ElevationRoughConfig(*GOOD_ROUGH)
    out = np.zeros(20, dtype=np.int8)
    cp, op = columns.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.ctypes.data_as(C.POINTER(C.c_byte))
    call = lib.kicp_elev_traversability_rough_from_columns
    assert call(None, 5, 4, C.byref(cfg), C.byref(slope), C.byref(rough), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, None, C.byref(slope), C.byref(rough), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, C.byref(cfg), None, C.byref(rough), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, C.byref(cfg), C.byref(slope), None, 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, C.byref(cfg), C.byref(slope), C.byref(rough), 0, 0, 5, 4, None, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 5, 4, C.byref(cfg), C.byref(slope), C.byref(rough), 0, 0, 5, 4, op, None, None, None, 19) == K.KICP_ERR_ARG
    assert call(cp, 0, 4, C.byref(cfg), C.byref(slope), C.byref(rough), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_ARG
    assert call(cp, 16385, 16384, C.byref(cfg), C.byref(slope), C.byref(rough), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_ERR_CAPACITY
    assert call(cp, 5, 4, C.byref(cfg), C.byref(slope), C.byref(rough), 0, 0, 5, 4, op, None, None, None, 20) == K.KICP_OK and (out == -1).all()
