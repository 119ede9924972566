"""The information gain without a GPU: the pure-host entry (K.gain_from_occupancy) against the restatement of include/kicp.h's text
(tests/gain_ref.py) - np.array_equal, no tolerance - the header's pinned 9 x 7 example with its rows written out, the walk's coverage of
the disc, the argument errors of the C and the Python entries, n_views == 0, and the shared header (kicp_gain_host.hpp: the arithmetic
the kernels call) in a stand-alone program, built plainly and under ASan + UBSan, on the same cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import gain_ref as gr

CASES = gr.cases()
PAIRS = sorted((name, R) for name, (_, _, ranges) in CASES.items() for R in ranges)


def test_pinned_9x7_example():
    occ, views, want = gr.pinned_9x7()
    assert occ.shape == (7, 9) and K.GAIN_WORDS == 4 == gr.WORDS
    indices = np.array([y * 9 + x for x, y in views], dtype=np.uint32)
    for R, rows in want.items():
        assert np.array_equal(gr.gain(occ, views, R), rows), R
        got = K.gain_from_occupancy(occ, np.array(views), R)  # (N, 2) of (x, y)
        assert got.dtype == np.uint32 and got.shape == (5, 4) and np.array_equal(got, rows), (R, got.tolist())
        assert np.array_equal(K.gain_from_occupancy(occ, indices, R), rows)  # cell indices
        assert np.array_equal(K.gain_from_occupancy(occ, indices.tolist(), R), rows)
    # duplicates give duplicate rows, in the order of the viewpoints
    twice = np.concatenate([indices[::-1], indices])
    assert np.array_equal(K.gain_from_occupancy(occ, twice, 3), np.concatenate([want[3][::-1], want[3]]))


@pytest.mark.parametrize("R", sorted(gr.EMPTY_PLANE_VISITS))
def test_the_rays_cover_the_disc_on_an_empty_plane(R):
    """the restatement's walk visits every offset of the disc but (0, 0), in the number of visits the header's text gives; on an all-
    unknown plane with a clear viewpoint the host entry therefore sees the whole disc"""
    visits = []
    side = 2 * R + 1
    assert gr.gain_one([[gr.CLEAR] * side for _ in range(side)], R, R, R, visits) == [0, 0, 0, 0]
    yy, xx = np.mgrid[-R:R + 1, -R:R + 1]
    disc = int((xx * xx + yy * yy <= R * R).sum()) - 1
    assert len(visits) == gr.EMPTY_PLANE_VISITS[R] and len(set(visits)) == disc and (0, 0) not in visits
    occ = np.full((side, side), -1, dtype=np.int8)
    occ[R, R] = 0
    assert K.gain_from_occupancy(occ, [(R, R)], R).tolist() == [[disc, 0, 0, 0]]


@pytest.mark.parametrize("name,R", PAIRS)
def test_gain_from_occupancy(name, R):
    occ, views, _ = CASES[name]
    want = gr.reference()[(name, R)]
    got = K.gain_from_occupancy(occ, views, R)
    assert got.dtype == np.uint32 and got.shape == (len(views), 4)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[:3], want[:3])
    cls = gr.classes(occ).reshape(-1)[gr.as_indices(views, occ.shape[1])]
    assert np.array_equal(got[:, 3], cls) and (got[cls != 0, :3] == 0).all()
    assert (got[:, 1].astype(np.int64) + got[:, 2] <= 8 * R).all()
    if name == "all_clear":
        assert (got[:, :2] == 0).all() and got[0, 2] > 0  # every ray completes or is LEFT; from a corner some are
    if name in ("all_unknown", "one_cell_unknown"):
        assert (got == [0, 0, 0, 1]).all()
    if name == "all_occupied":
        assert (got == [0, 0, 0, 2]).all()
    if name == "one_cell_clear":
        assert got.tolist() == [[0, 0, 4 if R == 1 else 8 * R, 0]]  # every first step is outside - but at R = 1 the four diagonal ones end at the disc first
    if name == "unknown_rings":
        assert got[0, 0] == {1: 4, 2: 12}.get(R, 24) and got[0, 1] == got[0, 2] == 0  # 24 cells that up to 160 rays cross: each once
    if name == "cap_361_in_40x40":
        assert got[0, 2] > 4 * 361 and got[0, 0] > 100  # most of the 8 R rays are LEFT (the others end at the disc or at an obstacle: none completes)
    if (name, R) == ("disc_edge_5_0", 5) or (name, R) == ("disc_edge_3_4", 5):
        assert got[0, 1] == 1  # on the disc's edge: the ray that ends there is BLOCKED
    if (name, R) == ("disc_beyond_4_4", 5):
        assert got[0, 1] == 0  # 32 > 25: no ray gets there
    if name == "shadow" and R == 15:
        assert 0 < got[0, 0] < want[2, 0]  # the wall shadows the unknown region from the near viewpoint


def test_classes_follow_the_thresholds():
    """min_observations is only checked by the host entry (the readout has it applied); occupied_thresh moves cells between clear and
    occupied: 66 is occupied at 0.65 and clear at 1, 1 is occupied at 0"""
    rng = np.random.default_rng(9)
    occ = rng.choice(np.array([-1, 0, 1, 40, 65, 66, 100], dtype=np.int8), (50, 70))
    occ[20:30, 30:40] = 0
    views = [(35, 25), (31, 21), (38, 28), (0, 0), (69, 49), (10, 10)]
    seen = {}
    for thresh in (0.0, 0.65, 1.0):
        want = gr.gain(occ, views, 12, thresh)
        assert np.array_equal(K.gain_from_occupancy(occ, views, 12, 3, thresh), want)
        seen[thresh] = want
    assert not np.array_equal(seen[0.0], seen[0.65]) and not np.array_equal(seen[0.65], seen[1.0]) and (seen[1.0][:, 1] == 0).all()


def _call(occ, cfg, views, n, out, cap, width=None, height=None):
    u32 = C.POINTER(C.c_uint)
    return K.lib().kicp_gain_from_occupancy(None if occ is None else occ.ctypes.data_as(C.POINTER(C.c_byte)), occ.shape[1] if width is None else width,
                                            occ.shape[0] if height is None else height, None if cfg is None else C.byref(cfg),
                                            None if views is None else views.ctypes.data_as(u32), n, None if out is None else out.ctypes.data_as(u32), cap)


def test_no_viewpoints():
    occ = gr.pinned_9x7()[0]
    for views in ([], np.zeros(0, dtype=np.uint32), np.zeros((0, 2), dtype=np.int64)):
        got = K.gain_from_occupancy(occ, views, 3)
        assert got.dtype == np.uint32 and got.shape == (0, 4)
    out = np.full(8, 77, dtype=np.uint32)
    cfg = K.GainConfig(1, 0.65, 3)
    assert _call(occ, cfg, None, 0, None, 0) == K.KICP_OK
    assert _call(occ, cfg, np.zeros(2, dtype=np.uint32), 0, out, 0) == K.KICP_OK and (out == 77).all()


def _code(fn, *a, **kw):
    with pytest.raises(K.KicpError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


def test_argument_errors():
    occ, views, want = gr.pinned_9x7()
    for kw in (dict(min_observations=0), dict(min_observations=-1), dict(min_observations=1 << 32), dict(occupied_thresh=-0.01), dict(occupied_thresh=1.01),
               dict(occupied_thresh=float("nan")), dict(range_cells=0), dict(range_cells=362), dict(range_cells=-1), dict(range_cells=1 << 32)):
        args = dict(range_cells=3)
        args.update(kw)
        assert _code(K.gain_from_occupancy, occ, views, **args)[0] == K.KICP_ERR_ARG, kw
    for bad in (np.zeros((0, 4), np.int8), np.zeros(4, np.int8), np.zeros((2, 2, 2), np.int8)):
        assert _code(K.gain_from_occupancy, bad, [0], 3)[0] == K.KICP_ERR_ARG
    # viewpoints outside the grid: as (x, y) and as indices - the C entry names the first bad one
    for bad in ([(3, 3), (9, 0)], [(3, 3), (0, 7)], [(-1, 0)], [5, -1], [1 << 32], [0.5, 2.0]):
        assert _code(K.gain_from_occupancy, occ, bad, 3)[0] == K.KICP_ERR_ARG, bad
    code, message = _code(K.gain_from_occupancy, occ, [5, 62, 63, 7, 900], 3)
    assert code == K.KICP_ERR_ARG and "viewpoint 2 " in message and "63" in message
    assert np.array_equal(K.gain_from_occupancy(occ, [62], 361)[0], gr.gain(occ, [62], 361)[0])  # the last cell and the largest range are fine

    cfg = K.GainConfig(1, 0.65, 3)
    v = np.array([y * 9 + x for x, y in views], dtype=np.uint32)
    out = np.full(24, 77, dtype=np.uint32)
    assert _call(occ, cfg, v, 5, out, 20) == K.KICP_OK and np.array_equal(out[:20].reshape(5, 4), want[3]) and (out[20:] == 77).all()
    bad_view = v.copy()
    bad_view[3] = 63
    for args in ((None, cfg, v, 5, out, 20), (occ, None, v, 5, out, 20), (occ, cfg, None, 5, out, 20), (occ, cfg, v, 5, None, 20), (occ, cfg, v, 5, out, 19),
                 (occ, cfg, v, 5, out, 24), (occ, cfg, v, 5, out, 5), (occ, cfg, v, 0, out, 20), (occ, K.GainConfig(0, 0.65, 3), v, 5, out, 20),
                 (occ, K.GainConfig(1, 1.5, 3), v, 5, out, 20), (occ, K.GainConfig(1, -0.5, 3), v, 5, out, 20), (occ, K.GainConfig(1, float("nan"), 3), v, 5, out, 20),
                 (occ, K.GainConfig(1, 0.65, 0), v, 5, out, 20), (occ, K.GainConfig(1, 0.65, 362), v, 5, out, 20), (occ, cfg, bad_view, 5, out, 20)):
        out[:] = 77
        assert _call(*args, width=9, height=7) == K.KICP_ERR_ARG
        assert (out == 77).all()  # nothing written
    assert b"viewpoint 3 " in K.lib().kicp_last_error()
    assert _call(occ, cfg, v, 5, out, 20, width=0, height=7) == K.KICP_ERR_ARG and _call(occ, cfg, v, 5, out, 20, width=9, height=0) == K.KICP_ERR_ARG
    assert _call(occ, cfg, v, 5, out, 20, width=1 << 15, height=(1 << 13) + 1) == K.KICP_ERR_CAPACITY
    assert _call(occ, cfg, v, (1 << 24) + 1, out, 20) == K.KICP_ERR_CAPACITY and (out == 77).all()  # refused by its count alone: nothing is read
    assert K.lib().kicp_grid_gain(None, C.byref(cfg), v.ctypes.data_as(C.POINTER(C.c_uint)), 5, out.ctypes.data_as(C.POINTER(C.c_uint)), 20) == K.KICP_ERR_ARG


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "gain_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_gain_host_stand_alone(tmp_path, flags):
    """gain_host:: in a program of its own (tests/cpp/gain_host_test.cpp), as a subprocess; the sanitizers run on this host program
    only.  The rows' buffer holds exactly the rows there are.  It also writes the perimeter offsets by ray index: the 8 R of the text,
    each once."""
    exe = _build(tmp_path, "gain_host_test", flags)
    runs = 0
    for name, R in PAIRS:
        occ, views, _ = CASES[name]
        H, W = occ.shape
        v = gr.as_indices(views, W).astype(np.uint32)
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            np.array([W, H, R, len(v)], dtype=np.uint32).tofile(f)
            np.array([0.65], dtype=np.float64).tofile(f), occ.tofile(f), v.tofile(f)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        raw = open(dst, "rb").read()
        assert len(raw) == 16 * len(v) + 64 * R
        assert np.array_equal(np.frombuffer(raw[:16 * len(v)], dtype=np.uint32).reshape(-1, 4), gr.reference()[(name, R)]), (name, R)
        offsets = [tuple(o) for o in np.frombuffer(raw[16 * len(v):], dtype=np.int32).reshape(-1, 2).tolist()]
        assert sorted(offsets) == sorted(gr.perimeter(R)), (name, R)
        runs += 1
    assert runs >= 60
