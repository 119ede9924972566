"""The transient obstacles without a GPU: the pure-host entry (K.transients_from_counts) against the restatement of include/kicp.h's
text (tests/transient_ref.py: endpoints from tests/grid_ref.py, components by a flood fill and by min-label sweeps, which must agree) -
np.array_equal, no tolerance - a pinned 8 x 6 case with its labels, rows, plane and statistics written out by hand, min_size, the
capacity convention, equal-distance ties of word 9, the argument errors, and the shared header (kicp_transient_host.hpp: the
arithmetic the kernels call) in a stand-alone program, built plainly and under ASan + UBSan, on the same scenes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import transient_cases as tc
import transient_ref as tr

CASES = tc.cases()


def _reference(s, **kw):
    return tr.transients(s["cfg"], s["counts"], s["points"], s["pose"], s["sensor"], **dict(s["params"], **kw))


def _host(s, **kw):
    """-> (rows, labels, stats, plane) of the host entry"""
    return K.transients_from_counts(s["counts"], s["args"], s["points"], s["pose"], s["sensor"], return_labels=True, return_stats=True, return_plane=True,
                                    **dict(s["params"], **kw))


@pytest.fixture(scope="module")
def reference():
    """name -> (rows, labels, plane, stats) by the restatement's flood fill - computed once"""
    return {name: _reference(s) for name, s in CASES.items()}


def test_pinned_8x6_case():
    s, want_labels, want_rows, want_plane, want_stats = tc.pinned_8x6()
    n, stats3, sensor = tr.returns(s["cfg"], s["points"], s["pose"], s["sensor"])
    assert sensor == (0, 0) and stats3 == want_stats[:3] and n[4, 2] == 9 and n[5, 7] == 1 and int(n.sum()) == 30
    flags = tr.transient_cells(s["counts"], n, 1, 65, 2)
    assert np.array_equal(flags, want_labels != tr.NONE)
    assert np.array_equal(tr.fr.labels_flood(flags), want_labels) and np.array_equal(tr.fr.labels_sweeps(flags), want_labels)
    assert np.array_equal(tr.rows_of(want_labels, n, sensor, 2), want_rows) and np.array_equal(tr.plane_of(want_labels, 2), want_plane)
    rows, labels, stats, plane = _host(s)
    assert rows.dtype == np.uint64 and rows.shape == (2, K.TRANSIENT_WORDS) and np.array_equal(rows, want_rows)
    assert labels.dtype == np.uint32 and labels.shape == (6, 8) and np.array_equal(labels, want_labels)
    assert plane.dtype == np.uint8 and plane.shape == (6, 8) and np.array_equal(plane, want_plane)
    assert stats == want_stats
    assert np.array_equal(K.transients_from_counts(s["counts"], s["args"], s["points"], s["pose"], s["sensor"], **s["params"]), want_rows)
    # min_size 1 adds the lone cell 36 to the rows and the plane; min_size 4 leaves none, and the labels stay
    rows, labels, _, plane = _host(s, min_size=1)
    assert rows[:, 0].tolist() == [9, 21, 36] and rows[2].tolist() == [36, 1, 2, 8, 8, 4, 4, 4, 4, (32 << 32) + 36] and np.array_equal(rows[:2], want_rows)
    assert np.array_equal(labels, want_labels) and np.array_equal(plane, (want_labels != tr.NONE).astype(np.uint8))
    rows, labels, _, plane = _host(s, min_size=4)
    assert rows.shape == (0, K.TRANSIENT_WORDS) and np.array_equal(labels, want_labels) and not plane.any()
    # one return is enough at min_points 1: cell 47 becomes a transient of its own
    assert _host(s, min_points=1, min_size=1)[0][:, 0].tolist() == [9, 21, 36, 47]
    # free_max 59 drops the busy cell 21 (readout 60) and B shrinks to cell 22
    rows = _host(s, free_max=59, min_size=1)[0]
    assert rows[:, 0].tolist() == [9, 22, 36] and rows[1].tolist() == [22, 1, 2, 12, 4, 6, 6, 2, 2, (40 << 32) + 22]


@pytest.mark.parametrize("name", sorted(CASES))
def test_transients_from_counts(name, reference):
    s = CASES[name]
    want_rows, want_labels, want_plane, want_stats = reference[name]
    assert np.array_equal(_reference(s, sweeps=True)[1], want_labels)  # the restatement's two ways agree
    rows, labels, stats, plane = _host(s)
    assert rows.dtype == np.uint64 and labels.dtype == np.uint32 and plane.dtype == np.uint8 and labels.shape == plane.shape == s["counts"].shape[:2]
    assert np.array_equal(labels, want_labels), np.argwhere(labels != want_labels)[:5]
    assert np.array_equal(rows, want_rows) and np.array_equal(plane, want_plane) and stats == want_stats
    assert (np.diff(rows[:, 0].astype(np.int64)) > 0).all() and int(plane.sum()) == int(rows[:, 1].sum())
    assert stats[0] >= stats[1] >= stats[2] >= stats[3] == int((labels != tr.NONE).sum())
    for min_size in (1, 3):
        want = _reference(s, min_size=min_size)
        got = _host(s, min_size=min_size)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[2]) and np.array_equal(got[1], want_labels)
    W = s["args"][3]
    if name in ("no_points", "no_transient", "sensor_far_outside", "random_1x1"):
        assert len(rows) == 0 and (labels == tr.NONE).all() and not plane.any()
    if name == "corner_pair_31_31_32_32":
        assert rows.tolist() == [[31 * 64 + 31, 2, 3, 2 * 31 + 32, 2 * 31 + 32, 31, 32, 31, 32, ((28 * 28 * 2) << 32) + 31 * 64 + 31]]
    if name == "corner_pair_32_31_31_32":
        assert rows[0, :3].tolist() == [31 * 64 + 32, 2, 4]
    if name == "along_a_tile_border":
        assert rows[:, 1].tolist() == [112, 52]
    if name == "two_blobs_touch_at_a_corner":
        assert rows[:, :3].tolist() == [[10 * W + 10, 8, 12]] and rows[0, 5:9].tolist() == [10, 13, 10, 13]
    if name == "two_apart":
        assert rows[:, 1].tolist() == [1, 1, 1]
    if name == "min_points_boundary":
        assert rows[:, :3].tolist() == [[40 * W + 40, 1, 3]]
    if name == "free_max_boundary":
        assert rows[:, 0].tolist() == [20 * W + 20]
    if name == "unknown_under_many_returns":
        assert rows[:, :3].tolist() == [[50 * W + 51, 1, 1]] and stats == (51, 51, 2, 1)
    if name == "min_observations_turns_unknown":
        assert rows[:, 0].tolist() == [40 * W + 40]
    if name == "skipped_returns":
        assert stats == (5, 3, 2, 2) and rows[:, 0].tolist() == [35 * W + 45, 36 * W + 6]
    if name == "sensor_outside_the_grid":
        assert rows[:, 0].tolist() == [30 * W + 2, 60 * W + 60] and rows[0, 9] == ((22 * 22) << 32) + 30 * W + 2
    if name == "5000_returns_in_one_cell":
        assert rows.tolist() == [[34 * W + 33, 2, 5007, 5000 * 33 + 7 * 34, 5007 * 34, 33, 34, 34, 34, ((30 * 30 + 31 * 31) << 32) + 34 * W + 33]]
    if name == "nearest_ties":
        ring = rows[rows[:, 1] == 4][0]
        assert ring[0] == 31 * W + 32 and ring[9] == (1 << 32) + 31 * W + 32 and ring[2] == 5
    if name == "random_64x64":
        assert len(rows) > 64  # more than the wrapper's first capacity


def _call(s, cfg, rows, cap_rows, n, labels=None, cap_labels=0, plane=None, cap_plane=0, stats=None, counts=True, grid=True, points=True, n_points=None, pose=True,
          sensor=True):
    u64, u32, u8, dp = C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint), C.POINTER(C.c_ubyte), C.POINTER(C.c_double)
    g = grid if isinstance(grid, K.GridConfig) else K.GridConfig(*s["args"])
    pts = np.ascontiguousarray(s["points"])
    return K.lib().kicp_transients_from_counts(s["counts"].ctypes.data_as(C.POINTER(C.c_ushort)) if counts else None, C.byref(g) if grid else None,
                                               pts.ctypes.data_as(dp) if points else None, len(pts) if n_points is None else n_points,
                                               s["pose"].ctypes.data_as(dp) if pose else None, np.ascontiguousarray(s["sensor"]).ctypes.data_as(dp) if sensor else None,
                                               None if cfg is None else C.byref(cfg), None if rows is None else rows.ctypes.data_as(u64), cap_rows,
                                               None if n is None else C.byref(n), None if labels is None else labels.ctypes.data_as(u32), cap_labels,
                                               None if stats is None else stats.ctypes.data_as(u64), None if plane is None else plane.ctypes.data_as(u8), cap_plane)


def test_capacity(reference):
    s = CASES["random_65x63"]
    want, _, want_plane, _ = reference["random_65x63"]
    T = len(want)
    assert T > 10
    cfg = K.TransientConfig(**s["params"])
    for cap in (0, 3, T - 1):
        rows, n, plane = np.full((T + 2, 10), 77, dtype=np.uint64), C.c_size_t(99), np.full(want_plane.shape, 9, dtype=np.uint8)
        assert _call(s, cfg, rows if cap else None, cap, n, plane=plane, cap_plane=plane.size) == K.KICP_ERR_CAPACITY
        assert n.value == T and np.array_equal(rows[:cap], want[:cap]) and (rows[cap:] == 77).all()
        assert np.array_equal(plane, want_plane)  # the plane does not depend on the rows' capacity
    for cap in (T, T + 2):
        rows, n = np.full((T + 2, 10), 77, dtype=np.uint64), C.c_size_t(99)
        assert _call(s, cfg, rows, cap, n) == K.KICP_OK and n.value == T and np.array_equal(rows[:T], want) and (rows[T:] == 77).all()
    n = C.c_size_t(99)
    assert _call(CASES["no_transient"], cfg, None, 0, n) == K.KICP_OK and n.value == 0
    assert _call(CASES["no_points"], cfg, None, 0, n, points=False) == K.KICP_OK and n.value == 0  # n == 0 needs no points


def _code(fn, *a, **kw):
    with pytest.raises(K.KicpError) as e:
        fn(*a, **kw)
    return e.value.code


def test_argument_errors():
    s = tc.pinned_8x6()[0]
    args = (s["counts"], s["args"], s["points"], s["pose"], s["sensor"])
    for kw in (dict(min_observations=0), dict(min_observations=-1), dict(min_observations=1 << 32), dict(free_max=101), dict(free_max=-1), dict(min_points=0),
               dict(min_size=0), dict(min_size=-3)):
        assert _code(K.transients_from_counts, *args, **kw) == K.KICP_ERR_ARG, kw
    assert _code(K.transients_from_counts, s["counts"][:5], *args[1:]) == K.KICP_ERR_ARG
    assert K.transients_from_counts(*args, free_max=0)[:, 0].tolist() == [9, 22, 36, 47]
    assert K.transients_from_counts(*args, free_max=100)[:, 0].tolist() == [9, 21, 36, 38]  # the occupied cell 38 too, joined to 47

    cfg = K.TransientConfig(1, 65, 2, 2)
    rows, labels, plane, n = np.zeros((8, 10), dtype=np.uint64), np.zeros(48, dtype=np.uint32), np.zeros(48, dtype=np.uint8), C.c_size_t(5)
    assert _call(s, cfg, rows, 8, n, labels, 48, plane, 48, np.zeros(4, dtype=np.uint64)) == K.KICP_OK and n.value == 2
    bad = [dict(cfg=None), dict(n=None), dict(rows=None), dict(cap_labels=47, labels=labels), dict(cap_labels=49, labels=labels), dict(cap_labels=48), dict(labels=labels),
           dict(cap_plane=47, plane=plane), dict(cap_plane=48), dict(plane=plane), dict(counts=False), dict(grid=False), dict(points=False), dict(pose=False),
           dict(sensor=False), dict(cfg=K.TransientConfig(0, 65, 2, 2)), dict(cfg=K.TransientConfig(1, 101, 2, 2)), dict(cfg=K.TransientConfig(1, 65, 0, 2)),
           dict(cfg=K.TransientConfig(1, 65, 2, 0))]
    for g in (K.GridConfig(0.0, 0.0, 0.0, 8, 6, 0.0, 1.0, 20.0), K.GridConfig(1.0, float("nan"), 0.0, 8, 6, 0.0, 1.0, 20.0), K.GridConfig(1.0, 0.0, 0.0, 0, 6, 0.0, 1.0, 20.0),
              K.GridConfig(1.0, 0.0, 0.0, 8, 0, 0.0, 1.0, 20.0), K.GridConfig(1.0, 0.0, 0.0, 8, 6, 1.0, 1.0, 20.0), K.GridConfig(1.0, 0.0, 0.0, 8, 6, 0.0, 1.0, 0.0)):
        bad.append(dict(grid=g))
    for kw in bad:
        n.value = 5
        call = dict(cfg=cfg, rows=rows, cap_rows=8, n=n)
        call.update(kw)
        assert _call(s, **call) == K.KICP_ERR_ARG, kw
        assert n.value == 0 or kw.get("n", n) is None, kw  # *out_n is 0 after an argument error
    assert _call(s, cfg, rows, 8, n, grid=K.GridConfig(1.0, 0.0, 0.0, 8, 6, 0.0, 1.0, 4096.5)) == K.KICP_ERR_CAPACITY  # a reach of 4097 cells
    assert _call(s, cfg, rows, 8, n, grid=K.GridConfig(1.0, 0.0, 0.0, 1 << 15, (1 << 13) + 1, 0.0, 1.0, 20.0), counts=True) == K.KICP_ERR_CAPACITY
    assert _call(s, cfg, rows, 8, n, n_points=0x7FFFFFF0 // 3 + 1) == K.KICP_ERR_CAPACITY and n.value == 0
    # the device entries check their arguments before they touch a device
    L, u64 = K.lib(), C.POINTER(C.c_ulonglong)
    for entry in (L.kicp_grid_transients, L.kicp_grid_transients_device):
        assert entry(None, None, 0, s["pose"].ctypes.data_as(C.POINTER(C.c_double)), s["pose"].ctypes.data_as(C.POINTER(C.c_double)), C.byref(cfg), rows.ctypes.data_as(u64), 8,
                     C.byref(n), None, 0, None) == K.KICP_ERR_ARG
    assert L.kicp_grid_transient_plane(None, plane.ctypes.data_as(C.POINTER(C.c_ubyte)), 48) == K.KICP_ERR_ARG
    assert L.kicp_grid_use_transients(None, 1) == K.KICP_ERR_ARG and L.kicp_grid_uses_transients(None) == 0


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "transient_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_transient_host_stand_alone(tmp_path, reference, flags):
    """transient_host:: in a program of its own (tests/cpp/transient_host_test.cpp), as a subprocess; the sanitizers run on this host
    program only.  The rows' buffer holds exactly the rows there are - or two, to see a short buffer handled"""
    exe = _build(tmp_path, "transient_host_test", flags)
    runs = 0
    for k, (name, s) in enumerate(sorted(CASES.items())):
        want, want_labels, want_plane, want_stats = reference[name]
        cfg, p = s["cfg"], s["params"]
        W, H = cfg["width"], cfg["height"]
        cap = 2 if k % 4 == 3 else len(want)
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            np.array([W, H, cfg["reach"], p["min_observations"], p["free_max"], p["min_points"], p["min_size"], cap], dtype=np.uint32).tofile(f)
            np.array([len(s["points"])], dtype=np.uint64).tofile(f)
            np.concatenate([[cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["z_min"], cfg["z_max"]], s["pose"], s["sensor"]]).astype(np.float64).tofile(f)
            s["counts"].tofile(f), np.ascontiguousarray(s["points"], dtype=np.float64).tofile(f)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (name, (out.stdout + out.stderr)[-2000:])
        raw = open(dst, "rb").read()
        stored = min(cap, len(want))
        head = np.frombuffer(raw[:40], dtype=np.uint64)
        assert int(head[0]) == len(want) and tuple(int(v) for v in head[1:]) == want_stats, name
        assert np.array_equal(np.frombuffer(raw[40:40 + 80 * stored], dtype=np.uint64).reshape(stored, 10), want[:stored]), name
        at = 40 + 80 * stored
        assert np.array_equal(np.frombuffer(raw[at:at + 4 * W * H], dtype=np.uint32).reshape(H, W), want_labels), name
        assert np.array_equal(np.frombuffer(raw[at + 4 * W * H:], dtype=np.uint8).reshape(H, W), want_plane), name
        runs += 1
    assert runs >= 25
