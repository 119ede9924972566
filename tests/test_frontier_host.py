"""The exploration frontiers without a GPU: the pure-host entry (K.frontiers_from_occupancy) against the restatement of include/kicp.h's
text (tests/frontier_ref.py: a flood fill and numpy min-label sweeps, which must agree) - np.array_equal, no tolerance - a pinned 8 x 6
case with its labels and rows written out by hand, min_size, the capacity convention, potentials with ties, the argument errors, and
the shared header (kicp_front_host.hpp: the arithmetic the kernels call) in a stand-alone program, built plainly and under ASan +
UBSan, on the same cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import frontier_ref as fr

CASES = fr.cases()


@pytest.fixture(scope="module")
def reference():
    """name -> (rows, labels) by the restatement's flood fill, without a potential - computed once"""
    return {name: fr.frontiers(occ) for name, occ in CASES.items()}


def test_pinned_8x6_case():
    occ, want_labels, want_rows = fr.pinned_8x6()
    flags = fr.frontier_cells(occ)
    assert np.array_equal(flags, want_labels != fr.NONE)
    assert np.array_equal(fr.labels_flood(flags), want_labels) and np.array_equal(fr.labels_sweeps(flags), want_labels)
    assert np.array_equal(fr.rows_of(want_labels), want_rows)
    rows, labels = K.frontiers_from_occupancy(occ, return_labels=True)
    assert rows.dtype == np.uint64 and rows.shape == (2, K.FRONTIER_WORDS) and np.array_equal(rows, want_rows)
    assert labels.dtype == np.uint32 and labels.shape == (6, 8) and np.array_equal(labels, want_labels)
    assert np.array_equal(K.frontiers_from_occupancy(occ), want_rows)
    # min_size drops the small frontier from the rows and not from the label plane
    rows, labels = K.frontiers_from_occupancy(occ, min_size=4, return_labels=True)
    assert np.array_equal(rows, want_rows[:1]) and np.array_equal(labels, want_labels)
    assert K.frontiers_from_occupancy(occ, min_size=9).shape == (0, K.FRONTIER_WORDS)
    # a potential: cells 12 and 14 tie at the least value of A - the lower index wins; B's least stands alone
    pot = (100 + np.arange(48, dtype=np.uint32)).reshape(6, 8)
    pot[1, 4] = pot[1, 6] = 7
    pot[4, 1] = 5
    want = want_rows.copy()
    want[0, 8:] = (7, 12)
    want[1, 8:] = (5, 33)
    assert np.array_equal(K.frontiers_from_occupancy(occ, potential=pot), want) and np.array_equal(fr.rows_of(want_labels, pot), want)
    # at occupied_thresh 0.5 the busy cell `f` is occupied, which changes no frontier; at 0 the cells of value 0 stay clear
    assert np.array_equal(K.frontiers_from_occupancy(occ, occupied_thresh=0.5), want_rows)
    assert np.array_equal(K.frontiers_from_occupancy(occ, occupied_thresh=0.0), want_rows)


@pytest.mark.parametrize("name", sorted(CASES))
def test_frontiers_from_occupancy(name, reference):
    occ = CASES[name]
    want_rows, want_labels = reference[name]
    flags = fr.frontier_cells(occ)
    assert np.array_equal(fr.labels_sweeps(flags), want_labels)  # the restatement's two ways agree
    rows, labels = K.frontiers_from_occupancy(occ, return_labels=True)
    assert rows.dtype == np.uint64 and labels.dtype == np.uint32 and labels.shape == occ.shape
    assert np.array_equal(labels, want_labels), np.argwhere(labels != want_labels)[:5]
    assert np.array_equal(rows, want_rows)
    assert int(rows[:, 1].sum()) == int(flags.sum()) and (np.diff(rows[:, 0].astype(np.int64)) > 0).all()
    assert (rows[:, 8] == fr.NONE).all() and np.array_equal(rows[:, 9], rows[:, 0])  # without a potential
    pot = fr.random_potential(occ.shape, len(name))
    for min_size in (1, 5):
        want = fr.rows_of(want_labels, pot, min_size)
        assert np.array_equal(K.frontiers_from_occupancy(occ, min_size=min_size, potential=pot), want)
    if name in ("all_unknown", "all_clear", "all_occupied", "one_cell_clear"):
        assert len(rows) == 0 and (labels == fr.NONE).all()
    if name == "single_clear_cell":
        assert rows.tolist() == [[820, 1, 20, 20, 20, 20, 20, 20, fr.NONE, 820]]
    if name == "corner_pair_31_31_32_32":
        assert rows.tolist() == [[31 * 64 + 31, 2, 63, 63, 31, 32, 31, 32, fr.NONE, 31 * 64 + 31]]
    if name == "corner_pair_32_31_31_32":
        assert rows.tolist() == [[31 * 64 + 32, 2, 63, 63, 31, 32, 31, 32, fr.NONE, 31 * 64 + 32]]
    if name == "two_apart":
        assert len(rows) == 6 and (rows[:, 1] == 1).all()
    if name == "along_a_tile_border":
        assert rows[:, 1].tolist() == [112, 52]
    if name == "serpentine_130x100":
        assert len(rows) == 1 and rows[0, 0] == 131 and rows[0, 1] == 25 * 128 + 24 * 3
    if name == "checkerboard_65":
        assert len(rows) == 1 and rows[0, 0] == 0 and rows[0, 1] == (65 * 65 + 1) // 2
    if name == "diamond_ring":
        assert len(rows) == 1 and rows[0, 0] == 20 * 96 + 48 and rows[0, 1] == 80 and rows[0, 4:8].tolist() == [28, 68, 20, 60]
    if name == "u_shape":
        assert len(rows) == 1 and rows[0, 0] == 3 * 70 + 50
    if name.startswith("random_130x100"):
        assert len(rows) >= 10 and rows[:, 1].max() > 1000  # 30 % unknown: one frontier runs through the whole grid, small ones beside it


def test_an_all_unreached_potential_equals_none():
    occ = CASES["random_70x50_seed1"]
    want = K.frontiers_from_occupancy(occ)
    assert np.array_equal(K.frontiers_from_occupancy(occ, potential=np.full(occ.shape, fr.NONE, dtype=np.uint32)), want)
    # equal potentials everywhere: every frontier's best cell is its least index, the label
    rows = K.frontiers_from_occupancy(occ, potential=np.full(occ.shape, 9, dtype=np.uint32))
    assert (rows[:, 8] == 9).all() and np.array_equal(rows[:, 9], rows[:, 0]) and np.array_equal(rows[:, :8], want[:, :8])


def _call(occ, cfg, rows, cap_rows, n, labels=None, cap_labels=0, potential=None, width=None, height=None):
    u64, u32 = C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)
    return K.lib().kicp_frontiers_from_occupancy(None if occ is None else occ.ctypes.data_as(C.POINTER(C.c_byte)), occ.shape[1] if width is None else width,
                                                 occ.shape[0] if height is None else height, None if cfg is None else C.byref(cfg),
                                                 None if potential is None else potential.ctypes.data_as(u32), None if rows is None else rows.ctypes.data_as(u64), cap_rows,
                                                 None if n is None else C.byref(n), None if labels is None else labels.ctypes.data_as(u32), cap_labels)


def test_capacity(reference):
    occ = CASES["random_70x50_seed2"]
    want, want_labels = reference["random_70x50_seed2"]
    F = len(want)
    assert F > 10
    cfg = K.FrontierConfig(1, 0.65, 1)
    for cap in (0, 3, F - 1):
        rows, n = np.full((F + 2, 10), 77, dtype=np.uint64), C.c_size_t(99)
        assert _call(occ, cfg, rows if cap else None, cap, n) == K.KICP_ERR_CAPACITY
        assert n.value == F and np.array_equal(rows[:cap], want[:cap]) and (rows[cap:] == 77).all()
    for cap in (F, F + 2):
        rows, n = np.full((F + 2, 10), 77, dtype=np.uint64), C.c_size_t(99)
        assert _call(occ, cfg, rows, cap, n) == K.KICP_OK and n.value == F and np.array_equal(rows[:F], want) and (rows[F:] == 77).all()
    # the filter counts before the capacity does
    big = fr.rows_of(want_labels, None, 5)
    rows, n = np.zeros((len(big), 10), dtype=np.uint64), C.c_size_t()
    assert 0 < len(big) < F and _call(occ, K.FrontierConfig(1, 0.65, 5), rows, len(big), n) == K.KICP_OK and n.value == len(big) and np.array_equal(rows, big)
    # no frontier at all: nothing needed, nothing stored
    n = C.c_size_t(99)
    assert _call(CASES["all_clear"], cfg, None, 0, n) == K.KICP_OK and n.value == 0
    # the wrapper's own second call: more frontiers than its first capacity
    occ = fr.in_unknown(120, 30, [(x, y) for x in range(1, 119, 3) for y in range(1, 29, 3)])
    rows = K.frontiers_from_occupancy(occ)
    assert len(rows) == 40 * 10 and np.array_equal(rows, fr.frontiers(occ)[0])


def _code(fn, *a, **kw):
    with pytest.raises(K.KicpError) as e:
        fn(*a, **kw)
    return e.value.code


def test_argument_errors():
    occ = CASES["pinned_8x6"]
    for kw in (dict(min_observations=0), dict(min_observations=-1), dict(min_observations=1 << 32), dict(occupied_thresh=-0.01), dict(occupied_thresh=1.01),
               dict(occupied_thresh=float("nan")), dict(min_size=0), dict(min_size=-3), dict(potential=np.zeros((6, 7), dtype=np.uint32))):
        assert _code(K.frontiers_from_occupancy, occ, **kw) == K.KICP_ERR_ARG, kw
    for bad in (np.zeros((0, 4), np.int8), np.zeros(4, np.int8), np.zeros((2, 2, 2), np.int8)):
        assert _code(K.frontiers_from_occupancy, bad) == K.KICP_ERR_ARG
    assert len(K.frontiers_from_occupancy(occ, min_observations=7, occupied_thresh=1.0)) == 2 and len(K.frontiers_from_occupancy(occ, occupied_thresh=0.0)) == 2

    cfg = K.FrontierConfig(1, 0.65, 1)
    rows, labels, n = np.zeros((8, 10), dtype=np.uint64), np.zeros(48, dtype=np.uint32), C.c_size_t(5)
    assert _call(occ, cfg, rows, 8, n, labels, 48) == K.KICP_OK and n.value == 2
    for args in ((None, cfg, rows, 8, n), (occ, None, rows, 8, n), (occ, cfg, rows, 8, None), (occ, cfg, None, 8, n), (occ, cfg, rows, 8, n, labels, 47),
                 (occ, cfg, rows, 8, n, labels, 49), (occ, cfg, rows, 8, n, None, 48), (occ, cfg, rows, 8, n, labels, 0), (occ, K.FrontierConfig(0, 0.65, 1), rows, 8, n),
                 (occ, K.FrontierConfig(1, 1.5, 1), rows, 8, n), (occ, K.FrontierConfig(1, -0.5, 1), rows, 8, n), (occ, K.FrontierConfig(1, 0.65, 0), rows, 8, n)):
        n.value = 5
        assert _call(*args, width=8, height=6) == K.KICP_ERR_ARG
        assert n.value == 0 or args[4] is None  # *out_n is 0 after an argument error
    assert _call(occ, cfg, rows, 8, n, width=0, height=6) == K.KICP_ERR_ARG and _call(occ, cfg, rows, 8, n, width=8, height=0) == K.KICP_ERR_ARG
    assert _call(occ, cfg, rows, 8, n, width=1 << 15, height=(1 << 13) + 1) == K.KICP_ERR_CAPACITY
    assert K.lib().kicp_grid_frontiers(None, C.byref(cfg), 0, rows.ctypes.data_as(C.POINTER(C.c_ulonglong)), 8, C.byref(n), None, 0) == K.KICP_ERR_ARG


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "front_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_front_host_stand_alone(tmp_path, reference, flags):
    """front_host:: in a program of its own (tests/cpp/front_host_test.cpp), as a subprocess; the sanitizers run on this host program
    only.  The rows' buffer holds exactly the rows there are - or three, to see a short buffer handled; every other case has a potential"""
    exe = _build(tmp_path, "front_host_test", flags)
    runs = 0
    for k, (name, occ) in enumerate(sorted(CASES.items())):
        _, want_labels = reference[name]
        H, W = occ.shape
        pot = fr.random_potential(occ.shape, k) if k % 2 else None
        min_size = 5 if k % 3 == 2 else 1
        want = fr.rows_of(want_labels, pot, min_size)
        cap = 3 if k % 4 == 3 else len(want)
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            np.array([W, H, min_size, 0 if pot is None else 1, cap], dtype=np.uint32).tofile(f)
            np.array([0.65], dtype=np.float64).tofile(f), occ.tofile(f)
            if pot is not None:
                pot.tofile(f)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        raw = open(dst, "rb").read()
        stored = min(cap, len(want))
        assert int(np.frombuffer(raw[:8], dtype=np.uint64)[0]) == len(want), name
        assert np.array_equal(np.frombuffer(raw[8:8 + 80 * stored], dtype=np.uint64).reshape(stored, 10), want[:stored]), name
        assert np.array_equal(np.frombuffer(raw[8 + 80 * stored:], dtype=np.uint32).reshape(H, W), want_labels), name
        runs += 1
    assert runs >= 30
