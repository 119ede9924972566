"""The grid's clearance and costmap without a GPU: the pure-host entries (K.clearance_from_occupancy, K.costmap_from_occupancy,
K.nav2_cost_table) against the numpy restatement of include/kicp.h's text (tests/clearance_ref.py) - np.array_equal, no tolerance -
their argument errors, and the shared header (kicp_clear_host.hpp: the very arithmetic the kernels call) in a stand-alone program,
built plainly and under ASan + UBSan, on the same cases.  The one comparison that is not exact is the Nav2 table's exp against
numpy's: see test_nav2_cost_table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import clearance_ref as cr

CASES = cr.host_cases()


@pytest.fixture(scope="module")
def reference():
    """(name, unknown_is_obstacle) -> the full-grid clearance by the restatement - computed once"""
    return {(name, uio): cr.clearance(occ, radius, unknown_is_obstacle=uio) for name, (occ, radius) in CASES.items() for uio in (False, True)}


def test_pinned_8x6_case_of_the_restatement():
    occ, radius, want, want_uio = cr.pinned_8x6()
    assert np.array_equal(cr.clearance(occ, radius), want)
    assert np.array_equal(cr.clearance(occ, radius, unknown_is_obstacle=True), want_uio)
    assert np.array_equal(K.clearance_from_occupancy(occ, radius), want)
    assert np.array_equal(K.clearance_from_occupancy(occ, radius, unknown_is_obstacle=True), want_uio)
    # the costs of row iy = 5 and of the column x = 7 with a table of 254, 253, 253, 152, 119, 86, 52, 0 ...
    table = cr.mixed_table(3)
    assert table.tolist() == [254, 253, 253, 152, 119, 86, 52, 0, 0, 0, 0]
    cost = K.costmap_from_occupancy(occ, table)
    assert cost[5].tolist() == [0, 0, 0, 0, 0, 0, 0, 255]  # clearance 9 and 10 cost nothing; the unknown cell stays 255
    assert cost[:, 6].tolist() == [119, 253, 254, 253, 119, 0]
    assert cost[3, 7] == 253 and cost[4, 7] == 86
    occ2 = occ.copy()
    occ2[3, 7], occ2[4, 7] = -1, -1  # unknown cells at clearance 2 (t = 253) and 5 (t = 86)
    assert K.costmap_from_occupancy(occ2, table)[3:5, 7].tolist() == [253, 255]
    assert K.costmap_from_occupancy(occ2, table, inflate_unknown=True)[3:5, 7].tolist() == [253, 86]
    assert K.costmap_from_occupancy(occ2, table, inflate_unknown=True)[5, 7] == 255  # t = 0 never replaces no-information


@pytest.mark.parametrize("name", sorted(CASES))
def test_clearance_from_occupancy(name, reference):
    occ, radius = CASES[name]
    for uio in (False, True):
        got = K.clearance_from_occupancy(occ, radius, unknown_is_obstacle=uio)
        assert got.dtype == np.uint16 and got.shape == occ.shape and np.array_equal(got, reference[name, uio])
        # the restatement's other brute force, which the GPU tests use where the list of sources is long
        assert np.array_equal(cr.clearance_by_offsets(occ, radius, unknown_is_obstacle=uio), reference[name, uio])
    far = radius * radius + 1
    if name in ("no_source", "one_cell_clear", "one_cell_unknown"):
        assert (reference[name, False] == far).all()
    if name in ("all_sources", "one_cell_source"):
        assert (reference[name, False] == 0).all()
    if name == "corners_r20":
        assert reference[name, False][0, 18] == 324 and reference[name, False][0, 17] == 289 and reference[name, False][14, 18] == far
    if name == "random_37x29_r254":
        assert reference[name, False].max() < far  # the radius covers the whole grid


@pytest.mark.parametrize("name", sorted(CASES))
def test_costmap_from_occupancy(name, reference):
    occ, radius = CASES[name]
    table = cr.mixed_table(radius)
    if radius >= 3:
        assert (table == 0).any() and ((table >= 1) & (table <= 252)).any() and (table == 253).any() and (table == 254).any()
    for uio in (False, True):
        for inflate in (False, True):
            got = K.costmap_from_occupancy(occ, table, unknown_is_obstacle=uio, inflate_unknown=inflate)
            assert got.dtype == np.uint8 and np.array_equal(got, cr.costmap(occ, table, 0.65, uio, inflate, clear=reference[name, uio]))
    if name == "random_37x29_r3":
        a, b = (K.costmap_from_occupancy(occ, table, inflate_unknown=i) for i in (False, True))
        assert ((a == 255) & (b > 0) & (b < 253)).any() and ((a == 255) & (b == 255)).any() and ((a == 253) & (occ < 0)).any()


@pytest.mark.parametrize("name", ["pinned_8x6", "corners_r20", "random_37x29_r3", "random_37x29_r254", "one_cell_source"])
def test_rectangles_equal_the_slice_of_the_full_result(name, reference):
    occ, radius = CASES[name]
    table = cr.mixed_table(radius)
    full_cost = cr.costmap(occ, table, unknown_is_obstacle=True, inflate_unknown=True, clear=reference[name, True])
    for rect in cr.rectangles(occ.shape[1], occ.shape[0]):
        x0, y0, w, h = rect
        got = K.clearance_from_occupancy(occ, radius, unknown_is_obstacle=True, rect=rect)
        assert got.shape == (h, w) and np.array_equal(got, reference[name, True][y0:y0 + h, x0:x0 + w]), rect
        got = K.costmap_from_occupancy(occ, table, unknown_is_obstacle=True, inflate_unknown=True, rect=rect)
        assert np.array_equal(got, full_cost[y0:y0 + h, x0:x0 + w]), rect


def test_thresholds_and_min_observations():
    occ = np.array([[64, 65, 66, 100, 0, -1, 1, 50]], dtype=np.int8)
    for thresh in (0.0, 0.5, 0.65, 0.655, 1.0):
        got = K.clearance_from_occupancy(occ, 1, occupied_thresh=thresh)
        assert np.array_equal(got, cr.clearance(occ, 1, thresh)), thresh
        assert np.array_equal(got[0] == 0, occ[0].astype(np.float64) > thresh * 100.0)
    assert (K.clearance_from_occupancy(occ, 1, occupied_thresh=1.0) == 2).all()  # nothing is above 100
    assert K.clearance_from_occupancy(occ, 1, occupied_thresh=0.0)[0].tolist() == [0, 0, 0, 0, 1, 1, 0, 0]  # 0 and unknown are not above 0


@pytest.mark.parametrize("cell,radius,inscribed,scaling", [(0.05, 20, 0.3, 3.0), (0.25, 4, 0.3, 10.0), (0.05, 254, 0.45, 1.5), (0.1, 1, 0.0, 0.0), (0.1, 7, 5.0, 3.0)])
def test_nav2_cost_table(cell, radius, inscribed, scaling):
    """Equal to numpy's, or off by one only where 252 * factor lies within 1e-9 of an integer: two libms may round exp differently,
    and the truncation to a byte amplifies that only there"""
    got = K.nav2_cost_table(cell, radius, inscribed, scaling)
    want, raw = cr.nav2_table(cell, radius, inscribed, scaling)
    assert got.dtype == np.uint8 and got.shape == (radius * radius + 2,)
    differs = got != want
    near = np.abs(raw - np.round(raw)) < 1e-9
    assert not (differs & ~near).any() and (np.abs(got.astype(int) - want.astype(int)) <= 1).all()
    assert got[0] == 254 and got[-1] == 0
    d = np.sqrt(np.arange(1, radius * radius + 1, dtype=np.float64)) * cell
    assert (got[1:-1][d <= inscribed] == 253).all() and (got[1:-1][d > inscribed] <= 252).all()
    assert (np.diff(got[1:-1].astype(int)) <= 0).all() and got[0] >= got[1]  # non-increasing in d2
    if scaling == 0.0:
        assert got.tolist() == [254, 252, 0]
    if inscribed >= radius * cell:
        assert (got[1:-1] == 253).all()


def _codes(fn, *variants):
    out = []
    for kw in variants:
        with pytest.raises(K.KicpError) as e:
            fn(**kw)
        out.append((e.value.code, str(e.value)))
    return out


def test_argument_errors():
    occ = np.zeros((4, 6), dtype=np.int8)
    table = cr.mixed_table(2)

    def clearance(radius_cells=2, **kw):
        return K.clearance_from_occupancy(occ, radius_cells, **kw)

    def costmap(table=table, **kw):
        return K.costmap_from_occupancy(occ, table, **kw)

    bad = [dict(min_observations=0), dict(occupied_thresh=-0.01), dict(occupied_thresh=1.01), dict(occupied_thresh=float("nan")), dict(rect=(0, 0, 7, 4)),
           dict(rect=(0, 0, 6, 5)), dict(rect=(6, 0, 1, 1)), dict(rect=(0, 4, 1, 1)), dict(rect=(2, 2, 0, 1)), dict(rect=(2, 2, 1, 0)), dict(rect=(5, 3, 2, 1)),
           dict(rect=(-1, 0, 2, 2))]
    assert all(c == K.KICP_ERR_ARG for c, _ in _codes(clearance, dict(radius_cells=0), dict(radius_cells=-3), *bad))
    (code, msg), = _codes(clearance, dict(radius_cells=255))
    assert code == K.KICP_ERR_CAPACITY and "254" in msg
    assert clearance(radius_cells=254).shape == (4, 6)
    assert all(c == K.KICP_ERR_ARG for c, _ in _codes(costmap, dict(table=table[:-1]), dict(table=np.zeros(1, np.uint8)), dict(table=np.zeros((2, 3), np.uint8)), *bad))
    (code, msg), = _codes(costmap, dict(table=np.zeros(255 * 255 + 2, np.uint8)))
    assert code == K.KICP_ERR_CAPACITY and "254" in msg
    for shape in ((0, 4), (4,), (2, 2, 2)):
        with pytest.raises(K.KicpError) as e:
            K.clearance_from_occupancy(np.zeros(shape, dtype=np.int8), 2)
        assert e.value.code == K.KICP_ERR_ARG

    # the C entries themselves: null pointers, cap != w * h, a table of the wrong length
    lib = K.lib()
    cfg = K.GridClearanceConfig(1, 0.65, 0, 2)
    i8, u8, u16 = C.POINTER(C.c_byte), C.POINTER(C.c_ubyte), C.POINTER(C.c_ushort)
    o16, o8 = np.zeros(24, dtype=np.uint16), np.zeros(24, dtype=np.uint8)
    po, pt, p16, p8 = occ.ctypes.data_as(i8), table.ctypes.data_as(u8), o16.ctypes.data_as(u16), o8.ctypes.data_as(u8)
    assert lib.kicp_grid_clearance_from_occupancy(po, 6, 4, C.byref(cfg), 0, 0, 6, 4, p16, 24) == K.KICP_OK
    assert lib.kicp_grid_clearance_from_occupancy(None, 6, 4, C.byref(cfg), 0, 0, 6, 4, p16, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clearance_from_occupancy(po, 6, 4, None, 0, 0, 6, 4, p16, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clearance_from_occupancy(po, 6, 4, C.byref(cfg), 0, 0, 6, 4, None, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clearance_from_occupancy(po, 6, 4, C.byref(cfg), 0, 0, 6, 4, p16, 23) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clearance_from_occupancy(po, 6, 4, C.byref(cfg), 1, 1, 2, 2, p16, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clearance_from_occupancy(po, 6, 4, C.byref(cfg), 0xFFFFFFFF, 0, 2, 1, p16, 2) == K.KICP_ERR_ARG  # x0 + w would wrap
    assert lib.kicp_grid_costmap_from_occupancy(po, 6, 4, C.byref(cfg), pt, 6, 0, 0, 0, 6, 4, p8, 24) == K.KICP_OK
    assert lib.kicp_grid_costmap_from_occupancy(None, 6, 4, C.byref(cfg), pt, 6, 0, 0, 0, 6, 4, p8, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap_from_occupancy(po, 6, 4, None, pt, 6, 0, 0, 0, 6, 4, p8, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap_from_occupancy(po, 6, 4, C.byref(cfg), None, 6, 0, 0, 0, 6, 4, p8, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap_from_occupancy(po, 6, 4, C.byref(cfg), pt, 6, 0, 0, 0, 6, 4, None, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap_from_occupancy(po, 6, 4, C.byref(cfg), pt, 5, 0, 0, 0, 6, 4, p8, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap_from_occupancy(po, 6, 4, C.byref(cfg), pt, 6, 0, 0, 0, 6, 4, p8, 25) == K.KICP_ERR_ARG
    assert lib.kicp_grid_cost_table_nav2(0.05, 2, 0.1, 3.0, pt, 6) == K.KICP_OK
    assert lib.kicp_grid_cost_table_nav2(0.05, 2, 0.1, 3.0, None, 6) == K.KICP_ERR_ARG
    assert lib.kicp_grid_cost_table_nav2(0.05, 2, 0.1, 3.0, pt, 5) == K.KICP_ERR_ARG
    assert lib.kicp_grid_cost_table_nav2(0.05, 0, 0.1, 3.0, pt, 2) == K.KICP_ERR_ARG
    assert lib.kicp_grid_cost_table_nav2(0.05, 255, 0.1, 3.0, pt, 255 * 255 + 2) == K.KICP_ERR_CAPACITY
    for cell, inscribed, scaling in ((0.0, 0.1, 3.0), (-0.05, 0.1, 3.0), (float("inf"), 0.1, 3.0), (float("nan"), 0.1, 3.0), (0.05, -0.1, 3.0), (0.05, float("nan"), 3.0),
                                     (0.05, 0.1, -1.0), (0.05, 0.1, float("inf"))):
        assert lib.kicp_grid_cost_table_nav2(cell, 2, inscribed, scaling, pt, 6) == K.KICP_ERR_ARG, (cell, inscribed, scaling)
    assert lib.kicp_grid_last_window(None, None, None, None, None) == K.KICP_ERR_ARG
    assert lib.kicp_grid_clearance(None, C.byref(cfg), 0, 0, 6, 4, p16, 24) == K.KICP_ERR_ARG
    assert lib.kicp_grid_costmap(None, C.byref(cfg), pt, 6, 0, 0, 0, 6, 4, p8, 24) == K.KICP_ERR_ARG


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "clear_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_clear_host_stand_alone(tmp_path, reference, flags):
    """clear_host:: in a program of its own (tests/cpp/clear_host_test.cpp), as a subprocess; the sanitizers run on this host program only"""
    exe = _build(tmp_path, "clear_host_test", flags)
    runs = 0
    for name, (occ, radius) in sorted(CASES.items()):
        H, W = occ.shape
        table = cr.mixed_table(radius)
        rects = cr.rectangles(W, H) if name in ("pinned_8x6", "random_37x29_r3", "random_37x29_r254") else [(0, 0, W, H)]
        for k, rect in enumerate(rects):
            uio, inflate = bool(k % 2), bool((k // 2) % 2) if k else True
            x0, y0, w, h = rect
            src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            with open(src, "wb") as f:
                np.array([W, H, 0.65, float(uio), radius, float(inflate), x0, y0, w, h, 0.05, 0.3, 3.0, 1], dtype=np.float64).tofile(f)
                occ.tofile(f), table.tofile(f)
            out = subprocess.run([exe, src, dst], capture_output=True, text=True)
            assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
            raw = open(dst, "rb").read()
            assert len(raw) == 3 * w * h + radius * radius + 2
            full = reference[name, uio]
            assert np.array_equal(np.frombuffer(raw[:2 * w * h], dtype=np.uint16).reshape(h, w), full[y0:y0 + h, x0:x0 + w]), (name, rect)
            want = cr.costmap(occ, table, 0.65, uio, inflate, clear=full)[y0:y0 + h, x0:x0 + w]
            assert np.array_equal(np.frombuffer(raw[2 * w * h:3 * w * h], dtype=np.uint8).reshape(h, w), want), (name, rect)
            assert np.array_equal(np.frombuffer(raw[3 * w * h:], dtype=np.uint8), K.nav2_cost_table(0.05, radius, 0.3, 3.0))
            runs += 1
    assert runs >= 20
