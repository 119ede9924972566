"""The fill of a grid's unknown cells from another grid without a GPU: that the cases (tests/grid_fill_cases.py) enter every pair of
classes and sit on both sides of every threshold; the pure-host entry (K.fill_unknown_counts) against the restatement
(tests/elev_rough_ref.py's fill); grid_host::fill_unknown in the stand-alone program of tests/cpp/elev_rough_host_test.cpp, built
plainly and under ASan + UBSan; and the argument errors.  Everything is exact."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
import elev_rough_ref as rr
import grid_fill_cases as fc
from test_elev_rough_host import BUILDS, _build


def test_the_table_holds_every_pair_and_both_sides_of_every_threshold():
    dst, src = fc.table()
    min_obs, free_max, occupied_min = fc.TABLE_CONFIG
    reads = rr.readout(np.array(fc.TABLE_SRC, dtype=np.uint16), min_obs)
    assert list(reads) == fc.TABLE_READS
    assert {free_max, free_max + 1, occupied_min - 1, occupied_min} <= set(fc.TABLE_READS)
    assert sum(fc.TABLE_SRC[1]) == min_obs and sum(fc.TABLE_SRC[0]) == min_obs - 1 and (65535, 65535) in fc.TABLE_SRC and (65535, 65535) in fc.TABLE_DST
    after, words = rr.fill(dst, src, *fc.TABLE_CONFIG)
    obstacle, traversable, unknown = (np.array([d[0] > 0 for d in fc.TABLE_DST]), np.array([d[0] == 0 and d[1] > 0 for d in fc.TABLE_DST]),
                                      np.array([d == (0, 0) for d in fc.TABLE_DST]))
    free, occupied = (reads >= 0) & (reads <= free_max), reads >= occupied_min
    for rows in (obstacle, traversable, unknown):  # the nine pairs, counters beyond 1 on both sides
        for columns in (free, occupied, ~free & ~occupied):
            assert rows.any() and columns.any()
    assert max(max(d) for d in fc.TABLE_DST if d[0] > 0) > 1 and max(max(d) for d in fc.TABLE_DST if d[0] == 0) > 1
    assert all(w > 0 for w in words) and sum(words[:5]) == dst.shape[0] * dst.shape[1]
    # kept words keep their bits; the unknown row is filled per column
    assert np.array_equal(after[~unknown], dst[~unknown])
    row = after[unknown][0]
    assert [tuple(int(v) for v in cell) for cell in row] == [(0, 1) if f else (1, 0) if o else (0, 0) for f, o in zip(free, occupied)]
    never, _ = rr.fill(dst, src, 4, 25, 101)
    assert not (never[unknown][0][:, 0] > 0).any() and np.array_equal(never[unknown][0][:, 1], after[unknown][0][:, 1])


@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c[0])
def test_host_entry_against_the_restatement(case):
    name, dst, src, cfg = case
    want, words = rr.fill(dst, src, *cfg)
    before = dst.copy()
    got, counts = K.fill_unknown_counts(dst, src, *cfg, return_counts=True)
    assert got.dtype == np.uint16 and np.array_equal(got, want) and counts == words and np.array_equal(dst, before)
    assert sum(counts[:5]) == dst.size // 2
    assert np.array_equal(K.fill_unknown_counts(dst, src, *cfg), want)  # without the counts
    # a second call leaves the counters equal, and counts the filled cells as kept
    again, second = K.fill_unknown_counts(got, src, *cfg, return_counts=True)
    assert np.array_equal(again, got) and second[2] == second[3] == 0 and second[4] == counts[4]
    assert second[0] == counts[0] + counts[3] and second[1] == counts[1] + counts[2]


@BUILDS
def test_fill_host_stand_alone(tmp_path, flags):
    """grid_host::fill_unknown in a program of its own, as a subprocess; the sanitizers run on this host program only"""
    exe = _build(tmp_path, "elev_rough_host_test", flags)
    path, out_path = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for name, dst, src, cfg in fc.cases():
        with open(path, "wb") as f:
            np.array([dst.size // 2] + list(cfg), dtype=np.float64).tofile(f)
            np.ascontiguousarray(dst).tofile(f)
            np.ascontiguousarray(src).tofile(f)
        out = subprocess.run([exe, "fill", path, out_path], capture_output=True, text=True)
        assert out.returncode == 0, (name, (out.stdout + out.stderr)[-2000:])
        want, words = rr.fill(dst, src, *cfg)
        assert tuple(int(v) for v in out.stdout.split()[1:]) == words, name
        assert np.array_equal(np.fromfile(out_path, dtype=np.uint16).reshape(dst.shape), want), name


def test_argument_errors():
    dst, src = fc.table()
    for cfg in ((0, 25, 65), (1, 101, 101), (1, 25, 25), (1, 30, 25), (1, 25, 102), (1, 100, 100), (1, 2 ** 32 - 1, 101)):
        with pytest.raises(K.KicpError) as e:
            K.fill_unknown_counts(dst, src, *cfg)
        assert e.value.code == K.KICP_ERR_ARG, cfg
    with pytest.raises(K.KicpError):
        K.fill_unknown_counts(dst, src[:4], 1, 25, 65)
    lib, cfg = K.lib(), K.GridFillConfig(1, 25, 65)
    d, s = dst.copy(), src.copy()
    u16 = C.POINTER(C.c_ushort)
    call = lib.kicp_grid_fill_unknown_counts
    assert call(None, s.ctypes.data_as(u16), 80, C.byref(cfg), None) == K.KICP_ERR_ARG
    assert call(d.ctypes.data_as(u16), None, 80, C.byref(cfg), None) == K.KICP_ERR_ARG
    assert call(d.ctypes.data_as(u16), s.ctypes.data_as(u16), 80, None, None) == K.KICP_ERR_ARG
    assert call(d.ctypes.data_as(u16), d.ctypes.data_as(u16), 80, C.byref(cfg), None) == K.KICP_ERR_ARG  # dst is src
    assert np.array_equal(d, dst) and np.array_equal(s, src)
    assert call(None, None, 0, C.byref(cfg), None) == K.KICP_OK  # no cells: nothing to point at
    assert call(d.ctypes.data_as(u16), s.ctypes.data_as(u16), 80, C.byref(cfg), None) == K.KICP_OK and np.array_equal(d, rr.fill(dst, src, 1, 25, 65)[0])
