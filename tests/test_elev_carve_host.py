"""The height columns' carve without a GPU: a case pinned cell by cell, every case of tests/elev_carve_cases.py proven to enter its
regime, the pure-host entry (K.elev_update_columns) against the restatement (tests/elev_carve_ref.py) on all of them, the passer-by
drive, the argument errors, and elev_host::update - the host restatement over the very arithmetic the kernels call
(kicp_elev_host.hpp) - in a stand-alone program, built plainly and under ASan + UBSan.  Everything is exact: np.array_equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import elev_carve_cases as ecc
import elev_carve_ref as ecr
import elev_cases as ec
import elev_ref as er


@pytest.mark.parametrize("keep_ground", [1, 0])
def test_pinned_8x6_case_cell_by_cell(keep_ground):
    cfg, start, points, pose, sensor, (G, W, keep), want, stats = ecc.pinned_8x6(keep_ground)
    assert ecr.sensor(cfg, pose, sensor) == (0, 0, 2)
    assert ecr.triples(cfg, points, pose, sensor) == (2, [(0, 3, 0), (4, 0, 6)], 2)
    assert [ecr.ray_slab(2, 6, 4, j) for j in range(9)] == [2, 3, 3, 4, 4, 5, 5, 6, 6] and [ecr.ray_slab(2, 0, 3, j) for j in range(7)] == [2, 2, 1, 1, 1, 0, 0]
    assert [ecr.step_mask(2, 6, 4, k, 0) for k in range(3)] == [0x0C, 0x18, 0x30] and [ecr.step_mask(2, 0, 3, k, 0) for k in range(2)] == [0x04, 0x06]
    for run in (lambda c: ecr.update(cfg, c, points, pose, sensor, G, W, keep), lambda c: ecr.update(cfg, c, points[::-1], pose, sensor, G, W, keep),
                lambda c: K.elev_update_columns(cfg, c, points, pose, sensor, G, W, keep)):
        got = start.copy()
        assert run(got) == stats
        for iy in range(cfg["height"]):
            for ix in range(cfg["width"]):
                assert int(got[iy, ix]) == want.get((ix, iy), 0), (ix, iy)
    again = got.copy()  # the same frame again: nothing is left to clear, nothing is new
    assert K.elev_update_columns(cfg, again, points, pose, sensor, G, W, keep) == stats[:4] + (0, 0, 2, 0, 0) and np.array_equal(again, got)


def test_step_masks_at_the_columns_ends():
    """step_mask in Python integers, where no shift can go wrong, against the vectorised masks of the restatement on every case"""
    assert ecr.step_mask(8, 120, 1, 0, 0) == ec.FULL & ~0xFF and ecr.step_mask(8, -9, 1, 0, 0) == 0x1FF and ecr.step_mask(70, 90, 6, 2, 3) == 0
    assert ecr.step_mask(-9, -20, 3, 1, 2) == 0 and ecr.step_mask(8, 8, 5, 2, 64) == ec.FULL and ecr.step_mask(0, 63, 1, 0, 0) == (1 << 33) - 1
    assert ecr.step_mask(40, 63, 2, 1, 11) == ec.FULL & ~((1 << 35) - 1)  # u(1) = 46, u(3) = 57: lo = 35, hi = 68
    for name in ("mask_reaching_bit_63", "mask_hi_64_and_above", "mask_lo_below_0", "sensor_above_and_below_the_column", "steep_rays", "widen_64"):
        case = ecc.reference(name)[0]
        for points, pose, sensor, (G, W, _) in case["frames"]:
            _, tri, ss = ecr.triples(case["cfg"], points, pose, sensor)
            want = [ecr.step_mask(ss, es, max(abs(dx), abs(dy)), k, W) for dx, dy, es in tri for k in range(max(max(abs(dx), abs(dy)) - G, 0))]
            assert [int(m) for m in ecr.steps(case["cfg"], points, pose, sensor, G, W)[3]] == want and len(want) > 0, name


@pytest.mark.parametrize("name", sorted(ecc.CASES))
def test_case_enters_its_regime_and_the_host_entry_equals_the_restatement(name):
    case, after, stats = ecc.reference(name)
    print(name, stats)
    assert case["enters"](case, stats)
    columns = case["start"].copy()
    for k, (points, pose, sensor, (G, W, keep)) in enumerate(case["frames"]):
        got = K.elev_update_columns(case["cfg"], columns, points, pose, sensor, G, W, keep)
        assert got == stats[k] and sum(got[:4]) == len(points), (name, k)
        assert np.array_equal(columns, after[k]), (name, k)
        shuffled = (after[k - 1] if k else case["start"]).copy()  # the SET of triples decides: the points in another order, each twice
        order = np.random.default_rng(k).permutation(np.repeat(np.arange(len(points)), 2))
        twice = K.elev_update_columns(case["cfg"], shuffled, points[order], pose, sensor, G, W, keep)
        assert np.array_equal(shuffled, after[k]) and twice[4:6] == got[4:6] and twice[7:] == got[7:], (name, k)


def test_passer_by_is_carved_away_and_the_static_scene_stays():
    plain, carved = ecc.passer_by_reference()
    cfg, (S, H), region = ecc.PASSER_CFG, ecc.PASSER_CLASSES, ecc.PASSER_REGION
    host = ecc.zeros(cfg)
    for points, pose, sensor in ecc.passer_by():
        K.elev_update_columns(cfg, host, points, pose, sensor, *ecc.PASSER_CARVE)
    assert np.array_equal(host, carved)
    cls_plain, cls_carved = K.traversability_from_columns(plain, S, H), K.traversability_from_columns(carved, S, H)
    _, counts = K.traversability_from_columns(carved, S, H, rect=(158, 142, 8, 8), return_counts=True)
    in_region = np.zeros(cls_plain.shape, dtype=bool)
    in_region[region] = True
    box_plain, box_carved = int((cls_plain[region] == 100).sum()), int((cls_carved[region] == 100).sum())
    lost = int(((cls_plain == 100) & (cls_carved != 100) & ~in_region).sum())
    gained = int(((cls_carved == 100) & (cls_plain != 100) & ~in_region).sum())
    static = int(((cls_plain == 100) & ~in_region).sum())
    print("box cells: plain %d, update %d (BODY %d); static obstacle cells %d, lost %d, gained %d" % (box_plain, box_carved, counts[2], static, lost, gained))
    assert box_plain == 16 and box_carved <= 2 and counts[2] == 0
    assert not ((cls_plain != -1) & (cls_carved == -1)).any()  # no known cell becomes unknown
    assert 100 * lost <= static and gained == 0


def test_argument_errors():
    cfg, start, points, pose, sensor, (G, W, keep), _, stats = ecc.pinned_8x6(1)
    for kw in (dict(widen_slabs=65), dict(keep_ground=2), dict(widen_slabs=0xFFFFFFFF)):
        columns = start.copy()
        with pytest.raises(K.KicpError) as e:
            K.elev_update_columns(cfg, columns, points, pose, sensor, **kw)
        assert e.value.code == K.KICP_ERR_ARG and np.array_equal(columns, start), kw
    for bad in (dict(cell=0.0), dict(slab=np.nan), dict(max_ray=np.inf), dict(origin_x=np.nan), dict(z_origin=np.inf), dict(width=0)):
        with pytest.raises(K.KicpError) as e:
            K.elev_update_columns(dict(ecc.layer_config(cfg), **bad), start.copy(), points, pose, sensor)
        assert e.value.code == K.KICP_ERR_ARG, bad
    with pytest.raises(K.KicpError) as e:
        K.elev_update_columns(dict(ecc.layer_config(cfg), cell=0.001), start.copy(), points, pose, sensor)  # reach 9 000
    assert e.value.code == K.KICP_ERR_CAPACITY
    with pytest.raises(K.KicpError) as e:
        K.elev_update_columns(cfg, start.astype(np.int64), points, pose, sensor)
    assert e.value.code == K.KICP_ERR_ARG
    lib, layer, carve = K.lib(), K.ElevationConfig(*[ecc.layer_config(cfg)[n] for n, _ in K.ElevationConfig._fields_]), K.ElevationCarveConfig(G, W, keep)
    columns, out = start.copy(), np.zeros(9, dtype=np.uint64)
    cp, op = columns.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.ctypes.data_as(C.POINTER(C.c_ulonglong))
    xp, pp, sp = points.ctypes.data_as(K._dp), pose.ctypes.data_as(K._dp), sensor.ctypes.data_as(K._dp)
    call = lib.kicp_elev_update_columns
    assert call(None, cp, 48, xp, 2, pp, sp, C.byref(carve), op) == K.KICP_ERR_ARG and call(C.byref(layer), None, 48, xp, 2, pp, sp, C.byref(carve), op) == K.KICP_ERR_ARG
    assert call(C.byref(layer), cp, 48, None, 2, pp, sp, C.byref(carve), op) == K.KICP_ERR_ARG and call(C.byref(layer), cp, 48, xp, 2, None, sp, C.byref(carve), op) == K.KICP_ERR_ARG
    assert call(C.byref(layer), cp, 48, xp, 2, pp, None, C.byref(carve), op) == K.KICP_ERR_ARG and call(C.byref(layer), cp, 48, xp, 2, pp, sp, None, op) == K.KICP_ERR_ARG
    assert call(C.byref(layer), cp, 47, xp, 2, pp, sp, C.byref(carve), op) == K.KICP_ERR_ARG and "48" in lib.kicp_last_error().decode()
    assert call(C.byref(layer), cp, 48, xp, 0x7FFFFFF0 // 3 + 1, pp, sp, C.byref(carve), op) == K.KICP_ERR_CAPACITY
    assert np.array_equal(columns, start) and not out.any()  # the refused calls changed nothing
    assert call(C.byref(layer), cp, 48, None, 0, pp, sp, C.byref(carve), None) == K.KICP_OK and np.array_equal(columns, start)  # n == 0, no statistics asked for
    assert call(C.byref(layer), cp, 48, xp, 2, pp, sp, C.byref(carve), op) == K.KICP_OK and tuple(int(v) for v in out) == stats


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "elev_carve_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_elev_carve_host_stand_alone(tmp_path, flags):
    """elev_host::update in a program of its own (tests/cpp/elev_carve_host_test.cpp), as a subprocess, on every case; the sanitizers
    run on this host program only"""
    exe = _build(tmp_path, "elev_carve_host_test", flags)
    for name in sorted(ecc.CASES):
        case, after, stats = ecc.reference(name)
        src, dst = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        ecc.write_case(src, case)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (name, (out.stdout + out.stderr)[-2000:])
        assert [tuple(int(v) for v in ln.split()[1:]) for ln in out.stdout.splitlines() if ln.startswith("frame ")] == stats, name
        got = np.fromfile(dst, dtype=np.uint64).reshape((len(after),) + after[0].shape)
        assert np.array_equal(got, np.stack(after)), name
