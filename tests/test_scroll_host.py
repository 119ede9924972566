"""The scroll without a GPU: the pure-host entries (K.shift_plane, K.follow_shift) against the restatement of include/kicp.h's text
(tests/scroll_ref.py) - np.array_equal, no tolerance - for elements of 1, 2, 4 and 8 bytes on the small shapes of tests/scroll_cases.py,
a hand-written table of the follow rule, the argument errors, and the shared header (kicp_scroll_host.hpp: the arithmetic the kernel
and the entries call) in a stand-alone program, built plainly and under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import scroll_cases as sc
import scroll_ref as sr


def _code(fn, *a, **kw):
    with pytest.raises(K.KicpError) as e:
        fn(*a, **kw)
    return e.value.code


def test_restatement_by_hand():
    """the restatement itself, on a plane small enough to write out"""
    p = np.arange(1, 13, dtype=np.uint8).reshape(3, 4)  # rows 1 2 3 4 / 5 6 7 8 / 9 10 11 12
    assert sr.shift(p, 1, 0).tolist() == [[2, 3, 4, 0], [6, 7, 8, 0], [10, 11, 12, 0]]  # dx > 0: column 0 leaves, an empty one enters high
    assert sr.shift(p, -1, 0).tolist() == [[0, 1, 2, 3], [0, 5, 6, 7], [0, 9, 10, 11]]
    assert sr.shift(p, 0, 2).tolist() == [[9, 10, 11, 12], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert sr.shift(p, 3, -1).tolist() == [[0, 0, 0, 0], [4, 0, 0, 0], [8, 0, 0, 0]]
    assert not sr.shift(p, 4, 0).any() and not sr.shift(p, 0, -3).any() and np.array_equal(sr.shift(p, 0, 0), p)
    assert sr.leaving_strips(2, -1, 4, 3) == ((0, 0, 2, 3), (2, 2, 2, 1)) and sr.leaving_strips(-1, 0, 4, 3) == ((3, 0, 1, 3), None)


@pytest.mark.parametrize("elem_bytes", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", sc.SMALL, ids=lambda s: "%dx%d" % s)
def test_shift_plane(shape, elem_bytes):
    width, height = shape
    p = sc.plane(width, height, elem_bytes)
    for dx, dy in sc.shifts(width, height):
        got = K.shift_plane(p, dx, dy)
        assert got.dtype == p.dtype and got.shape == p.shape and np.array_equal(got, sr.shift(p, dx, dy)), (dx, dy)
        if abs(dx) >= width or abs(dy) >= height:
            assert not got.any(), (dx, dy)
    assert np.array_equal(K.shift_plane(p, 0, 0), p)


def test_shift_plane_pairs_and_columns():
    """the layouts the handles hold: counter pairs as one 32-bit element per cell, columns as 64-bit ones"""
    c, col = sc.counters(37, 29), sc.columns(37, 29)
    for dx, dy in ((4, -6), (-5, 3), (36, 28), (0, -1)):
        assert np.array_equal(K.shift_plane(c, dx, dy), sr.shift(c, dx, dy)) and np.array_equal(K.shift_plane(col, dx, dy), sr.shift(col, dx, dy))
    assert (sr.shift(col, 1, 1) >> np.uint64(63)).any()  # bit 63 travels


def test_shift_plane_argument_errors():
    L = K.lib()
    a, b = np.ones((4, 4), dtype=np.uint32), np.zeros((4, 4), dtype=np.uint32)
    call = lambda i, o, w=4, h=4, e=4, dx=1, dy=0: L.kicp_shift_plane(i, o, w, h, e, dx, dy)  # noqa: E731
    assert call(a.ctypes.data, b.ctypes.data) == K.KICP_OK and b[0].tolist() == [1, 1, 1, 0]
    assert call(None, b.ctypes.data) == K.KICP_ERR_ARG and call(a.ctypes.data, None) == K.KICP_ERR_ARG
    for e in (0, 3, 5, 16):
        assert call(a.ctypes.data, b.ctypes.data, e=e) == K.KICP_ERR_ARG, e
    assert call(a.ctypes.data, b.ctypes.data, w=0) == K.KICP_ERR_ARG and call(a.ctypes.data, b.ctypes.data, h=0) == K.KICP_ERR_ARG
    assert call(a.ctypes.data, b.ctypes.data, w=1 << 15, h=(1 << 13) + 1, e=1) == K.KICP_ERR_CAPACITY
    big = np.zeros(40, dtype=np.uint32)
    assert call(big.ctypes.data, big.ctypes.data) == K.KICP_ERR_ARG  # the same memory
    assert call(big.ctypes.data, big.ctypes.data + 4 * 15) == K.KICP_ERR_ARG and call(big.ctypes.data + 4 * 15, big.ctypes.data) == K.KICP_ERR_ARG  # one element shared
    assert call(big.ctypes.data, big.ctypes.data + 4 * 16) == K.KICP_OK  # back to back
    assert _code(K.shift_plane, np.zeros((0, 4), dtype=np.uint8), 0, 0) == K.KICP_ERR_ARG and _code(K.shift_plane, np.zeros(4, dtype=np.uint8), 0, 0) == K.KICP_ERR_ARG
    assert _code(K.shift_plane, np.zeros((2, 2, 3), dtype=np.uint8), 0, 0) == K.KICP_ERR_ARG  # 3 bytes per cell


# (c, size, margin, step) -> d, written out by hand for a 100-cell axis with a band of [10, 90) and steps of 16
FOLLOW_TABLE = [
    ((10, 100, 10, 16), 0), ((89, 100, 10, 16), 0), ((50, 100, 10, 16), 0),  # both edges of the band, and inside
    ((9, 100, 10, 16), -16), ((90, 100, 10, 16), 16),  # one cell outside: one step
    ((-6, 100, 10, 16), -16), ((-7, 100, 10, 16), -32),  # 16 short: one step; 17 short: two
    ((105, 100, 10, 16), 16), ((106, 100, 10, 16), 32),  # c - 90 + 1 = 16: one step; 17: two
    ((0, 100, 10, 16), -16), ((99, 100, 10, 16), 16), ((-1, 100, 10, 16), -16),
    ((-100000, 100, 10, 16), -16 * 6251), ((100000, 100, 10, 16), 16 * 6245),  # far outside on both sides: ceil(100010 / 16), ceil(99911 / 16)
    ((-(1 << 40), 100, 10, 1), -(1 << 40) - 10), ((1 << 40, 100, 10, 1), (1 << 40) - 89),
    ((0, 3, 1, 1), -1), ((1, 3, 1, 1), 0), ((2, 3, 1, 1), 1),  # the smallest axis the rule takes: the band is one cell
    ((0, 36, 10, 16), -16), ((35, 36, 10, 16), 16),  # 2 * margin + step == size: accepted
]


def test_follow_shift_table():
    for args, want in FOLLOW_TABLE:
        assert sr.follow_shift(*args) == want, args  # the restatement against the hand-written value
        assert K.follow_shift(*args) == want, args
    for bad in ((5, 35, 10, 16), (5, 100, 0, 16), (5, 100, 10, 0), (5, 2, 1, 1), (5, 0, 1, 1), (5, 100, 50, 1)):  # one above the boundary, margin 0, step 0, ...
        assert sr.follow_shift(*bad) is None and _code(K.follow_shift, *bad) == K.KICP_ERR_ARG, bad
    assert K.follow_shift(5, 100, 49, 2) == -44  # 2 * 49 + 2 == 100
    assert K.lib().kicp_follow_shift(5, 100, 10, 16, None) == K.KICP_ERR_ARG
    assert _code(K.follow_shift, -(1 << 63), 1 << 28, 1 << 26, 1 << 27) == K.KICP_ERR_ARG  # the shift would leave 64 bits


def test_follow_shift_lands_in_the_band():
    for size, margin, step in ((100, 10, 16), (36, 10, 16), (3, 1, 1), (64, 1, 62), (1600, 400, 64), (29, 7, 15)):
        for c in list(range(-3 * size, 4 * size)) + [-(1 << 31), 1 << 31, -12345678901, 12345678901]:
            d = K.follow_shift(c, size, margin, step)
            assert d == sr.follow_shift(c, size, margin, step) and d % step == 0 and margin <= c - d < size - margin, (c, size, margin, step, d)
            if margin <= c < size - margin:
                assert d == 0
            else:  # the least multiple that does: one step less falls short
                assert not margin <= c - (d - step if d > 0 else d + step) < size - margin


def _build(tmp_path, flags):
    exe = str(tmp_path / "scroll_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "scroll_host_test.cpp"), "-o", exe] + flags)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_scroll_host_stand_alone(tmp_path, flags):
    """kicp_scroll_host.hpp in a program of its own (tests/cpp/scroll_host_test.cpp), as a subprocess; the sanitizers run on this host
    program only"""
    exe = _build(tmp_path, flags)
    follow = [a for a, _ in FOLLOW_TABLE] + [(5, 35, 10, 16), (5, 100, 0, 16), (-(1 << 63), 1 << 28, 1 << 26, 1 << 27)]
    origins = [(-40.0, 64, 0.05), (0.1, -3, 0.1), (1e300, 2147483647, 1e300), (-12.35, 7, 0.05), (3.0000000000000004, -2147483648, 1e-9)]
    windows = [(5, -7, 3, 2), (-(1 << 30), 0, 7, 0), (0, 1 << 30, 0, -1), (100, 5, -2147483648, 0), (5, -100, 0, 2147483647), (0, 0, 0, 0), (-(1 << 30) + 7, (1 << 30) - 1, 7, -1)]
    runs = 0
    for width, height in sc.SMALL:
        for elem in (1, 2, 4, 8):
            p, shifts = sc.plane(width, height, elem), sc.shifts(width, height)
            src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            with open(src, "wb") as f:
                np.array([width, height, elem, len(shifts), len(follow), len(origins), len(windows), 0], dtype=np.uint32).tofile(f)
                np.array(shifts, dtype=np.int32).tofile(f), np.array(follow, dtype=np.int64).tofile(f)
                np.array(origins, dtype=np.float64).tofile(f), np.array(windows, dtype=np.int32).tofile(f), p.tofile(f)
            out = subprocess.run([exe, src, dst], capture_output=True, text=True)
            assert out.returncode == 0, ((width, height, elem), (out.stdout + out.stderr)[-2000:])
            raw = open(dst, "rb").read()
            planes = np.frombuffer(raw[:p.nbytes * len(shifts)], dtype=p.dtype).reshape(len(shifts), height, width)
            for k, (dx, dy) in enumerate(shifts):
                assert np.array_equal(planes[k], sr.shift(p, dx, dy)), (width, height, elem, dx, dy)
            at = p.nbytes * len(shifts)
            got = np.frombuffer(raw[at:at + 16 * len(follow)], dtype=np.int64).reshape(-1, 2)
            for (ok, d), args in zip(got.tolist(), follow):
                want = sr.follow_shift(*args) if abs(args[0]) < 1 << 62 else None
                assert (ok, d) == ((0, 0) if want is None else (1, want)), args
            at += 16 * len(follow)
            got = np.frombuffer(raw[at:at + 8 * len(origins)], dtype=np.float64)
            for g, (o, d, cell) in zip(got, origins):
                w = sr.origin(o, d, cell)
                assert g == w or (np.isinf(g) and np.isinf(w)), (o, d, cell)
            at += 8 * len(origins)
            got = np.frombuffer(raw[at:], dtype=np.int32).tolist()
            want = []
            for x0, y0, dx, dy in windows:  # the corner minus the shift; a corner beyond +-2^30 forgets the window and leaves the corner
                kept = abs(x0 - dx) <= 1 << 30 and abs(y0 - dy) <= 1 << 30
                want += [1, x0 - dx, y0 - dy] if kept else [0, x0, y0]
            assert got == want
            runs += 1
    assert runs == 32
