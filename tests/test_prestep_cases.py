"""The premises of tests/prestep_cases.py, proved on the CPU from the oracle alone, so that the regime each case of
tests/test_gpu_presteps_regimes.py claims - a bucket count, a tile count, a workgroup count, a hit or a miss of the guess - is a
property of its input and not something the device is trusted to report: the oracle's three survivor counts equal the table's and
a plain numpy count, no decision is borderline, and the bucket and tile counts the counts imply are the ones the case is named
after.  The range-error clouds: the oracle keeps what the device's table cannot express."""
import numpy as np
import pytest

import prestep_cases as pc
from oracle import okicp


def test_the_bucket_count_restated():
    """reference_bucket_count: ceil(float(n) / 0.5f) rounded up to a power of two - a count of 2^k keeps 2^(k+1) buckets, one more
    takes 2^(k+2)"""
    assert [pc.buckets(n) for n in (0, 1, 2, 3, 300, 6000, 300001)] == [0, 2, 4, 8, 1024, 16384, 1048576]
    for k in range(0, 20):
        assert pc.buckets(1 << k) == 2 << k and pc.buckets((1 << k) + 1) == 4 << k
    assert pc.table_tiles(0) == 0 and pc.table_tiles(1) == 1 and pc.table_tiles(128) == 1 and pc.table_tiles(129) == 2


@pytest.mark.parametrize("case", pc.FRAME_CASES, ids=repr)
def test_counts_and_margins_of_a_frame_case(case):
    pts = case.build()
    assert pts.shape == (case.n_in, 3)
    b0, b1, b2 = pc.oracle_chain(case)
    counts = pc.numpy_counts(pts, case.max_range, case.min_range, case.voxel_a, case.voxel_b)
    assert [len(b0), len(b1), len(b2)] == case.counts == counts
    assert case.counts[:2] == [case.n0, case.n1]  # (pinned in the table, not counted)
    # no borderline decision: ranges a metre and more from either bound, survivors in the middle third of their 0.5 m voxel (which
    # is the middle of a ninth of their 1.5 m voxel)
    r = np.sqrt((pts * pts).sum(axis=1))
    assert np.all((np.abs(r - case.max_range) > 1.0) & (np.abs(r - case.min_range) > 1.0))
    assert np.array_equal(b0, pts[r < case.max_range])  # identity poses, no deskew: the survivors themselves, in input order
    for v in (case.voxel_a, case.voxel_b):
        frac = b0 / v - np.floor(b0 / v)
        assert np.all((frac > 0.1) & (frac < 0.9))
    assert np.all(np.abs(np.floor(b0 / case.voxel_b)) < 1 << 20)
    if case.n0 > case.n1 > 0:  # duplicates differ from the point their voxel keeps
        assert len(np.unique(b0, axis=0)) == case.n0


def test_the_regimes_follow_from_the_counts():
    small = pc.SMALL_TABLE_BUCKETS
    # second level, several tiles per workgroup: 32 workgroups behind the 300-point frame, 64 tiles, a right guess
    c = pc.L2_SEVERAL_TILES
    assert pc.ORDINARY.n_in == 300 and c.n_in == 20000 and c.n1 > 4096 and c.hit
    assert pc.l2_workgroups(c.n_in, pc.ORDINARY.n1) == 32 and c.l2_tiles == 64 and c.point_tiles <= pc.SCAN_BLOCKS
    # second level, workgroups without a tile: several hundred for one tile, for none
    for c in (pc.ONE_VOXEL, pc.EMPTIED):
        assert c.guess is None and c.hit and pc.l2_workgroups(c.n_in, None) == 512
    assert pc.ONE_VOXEL.counts == [40000, 1, 1] and pc.ONE_VOXEL.l2_tiles == 1
    assert pc.EMPTIED.counts == [0, 0, 0] and pc.EMPTIED.l2_tiles == 0
    # point tiles against table tiles, either way round, both with a right guess
    assert pc.FEW_SURVIVE.hit and (pc.FEW_SURVIVE.point_tiles, pc.FEW_SURVIVE.l1_tiles) == (157, 8)
    assert pc.UNCROPPED.hit and (pc.UNCROPPED.point_tiles, pc.UNCROPPED.l1_tiles) == (157, 512) and pc.UNCROPPED.n0 == pc.UNCROPPED.n_in
    # small and window tables, at both levels (table A: of n0 points, table B: of n1)
    assert tuple(c.n0 for c in pc.SMALL_CASES) == pc.SMALL_COUNTS == (1, 2, 127, 128, 129, 255, 256, 257)
    for c in pc.SMALL_CASES:
        assert c.hit and c.n1 == c.n0 and c.l1_tiles == pc.table_tiles(c.n0)
        assert (pc.buckets(c.n0) <= small) == (c.n0 <= 256)
    assert pc.buckets(256) == small and pc.buckets(257) == 2 * small
    c = pc.SMALL_B
    assert c.hit and pc.buckets(c.n0) == 16384 > small and pc.buckets(c.n1) == small and c.l2_tiles == 2
    # bracket edges: of the four pairs two are hits
    assert [(c.n0, c.guess) for c in pc.EDGE_CASES] == [(4096, 4096), (4096, 4097), (4097, 4096), (4097, 4097), (256, 256), (256, 257), (257, 256), (257, 257)]
    assert [c.hit for c in pc.EDGE_CASES] == [True, False, False, True] * 2
    for c in pc.EDGE_CASES:
        assert c.n1 == c.n0 and c.hit == (c.n0 == c.guess)  # (table B sits on the same edge)
        assert c.spec_buckets() == (4 if c.guess & 1 else 2) * (c.guess & ~1)
    # hopeless guess: two buckets for 20 000 voxels, then the right table
    assert pc.HOPELESS.spec_buckets() == 2 and not pc.HOPELESS.hit and pc.HOPELESS.n1 == 20000
    assert pc.HOPELESS_THEN_RIGHT.hit and pc.HOPELESS_THEN_RIGHT.counts[:2] == pc.HOPELESS.counts[:2]
    assert not np.array_equal(pc.oracle_chain(pc.HOPELESS)[2][:8], pc.oracle_chain(pc.HOPELESS_THEN_RIGHT)[2][:8])  # another cloud
    assert pc.l2_workgroups(20000, 0) == 32 < pc.HOPELESS_THEN_RIGHT.l2_tiles == 256  # (a missed frame leaves one tile behind)
    # every frame case but the big one is one the chain fuses
    assert all(c.point_tiles <= pc.SCAN_BLOCKS for c in pc.FRAME_CASES)


def test_the_big_frame_and_its_prefixes():
    """Beyond 4 096 workgroups: the smallest sizes that enter the branch, with duplicates and a crop that bite."""
    big = pc.BIG
    pts = big.build()
    b0, b1, b2 = pc.oracle_chain(big)
    n0, n1, n2 = len(b0), len(b1), len(b2)
    assert [n0, n1, n2] == pc.numpy_counts(pts, big.max_range, big.min_range, big.voxel_a, big.voxel_b)
    assert pc.tiles(big.n_in) == pc.SCAN_BLOCKS + 1  # Preprocess: the separate scan; Frame: not fused
    assert pc.tiles(pc.buckets(big.n_in)) > pc.SCAN_BLOCKS  # ... and both gathers of the unfused chain scan too: three launches
    assert 0.3 * big.n_in < n0 < 0.6 * big.n_in and 0.8 * n0 < n1 < 0.95 * n0 and 0 < n2 < n1
    r = np.sqrt((pts * pts).sum(axis=1))
    assert np.all((np.abs(r - big.max_range) > 1e-7) & (np.abs(r - big.min_range) > 1e-7))
    assert np.abs(pts).max() <= 200.0  # voxel coordinates within +-400: far inside +-2^20
    # the stand-alone downsample: 524 288 points are the last to fit 4 096 table tiles; one more doubles the table, and the scan
    # kernel's loop (1 024 blocks a turn) takes eight turns
    assert pc.tiles(pc.buckets(pc.VD_LAST_FUSED)) == pc.SCAN_BLOCKS and pc.tiles(pc.buckets(pc.VD_FIRST_SCANNED)) == 2 * pc.SCAN_BLOCKS
    for n in (pc.VD_LAST_FUSED, pc.VD_FIRST_SCANNED):
        out = pc.oracle_downsample_of_big_prefix(n)
        assert 0.9 * n < len(out) < 0.99 * n and len(out) == pc.numpy_counts(pts[:n], 1e9, -1.0, pc.VOXEL_A, pc.VOXEL_B)[1]


def _pack21(v):
    """kicp_pre.hpp pack_voxel21: (in range, key of the coordinates masked to 21 bits)"""
    lim = 1 << 20
    ok = all(-lim <= int(c) < lim for c in v)
    return ok, sum(((int(c) + lim) & 0x1FFFFF) << (21 * a) for a, c in enumerate(v))


@pytest.mark.parametrize("axis,sign,k", pc.TWIN_CASES)
def test_the_twin_is_a_voxel_of_its_own_that_packs_like_its_neighbour(axis, sign, k):
    pts = pc.twin_cloud(axis, sign, k)
    vox = np.floor(pts / pc.VOXEL_A)
    ok_a, key_a = _pack21(vox[k])
    ok_b, key_b = _pack21(vox[k + 1])
    assert tuple(vox[k]) == pc.TWIN_VOXEL and ok_a and not ok_b and key_a == key_b
    assert k // 64 == (k + 1) // 64 or (k + 1) % 64 == 0  # both inside one wave, or the twin first of its wave
    assert all(_pack21(v)[0] for i, v in enumerate(vox) if i != k + 1)
    out = okicp.voxel_downsample(pts, pc.VOXEL_A)
    assert len(out) == pc.RANGE_N and len(np.unique(vox, axis=0)) == pc.RANGE_N  # the reference keeps the twin
    r = np.sqrt((pts * pts).sum(axis=1))
    assert np.all((r > pc.MIN_RANGE + 1.0) & (r < pc.FAR_RANGE / 2))  # nothing is cropped


def test_the_issues_example_and_the_other_range_clouds():
    out = okicp.voxel_downsample(np.array([[2.6, .1, .1], [(5 + 2**21 + .2) * .5, .1, .1], [2.7, .1, .1]]), 0.5)
    assert len(out) == 2
    # the reference converts a NaN coordinate to INT_MIN: three points, three voxels
    out = okicp.voxel_downsample(np.array([[.1, .1, .1], [np.nan, .1, .1], [.2, .1, np.nan]]), 0.5)
    assert len(out) == 3
    for value in pc.NONFINITE:
        for axis in range(3):
            pts = pc.nonfinite_cloud(value, axis, 10)
            assert np.flatnonzero(~np.isfinite(pts).all(axis=1)).tolist() == [10]
            rest = np.delete(pts, 10, axis=0)
            assert all(_pack21(v)[0] for v in np.floor(rest / pc.VOXEL_A))
    # the second level alone leaves the range
    pts = pc.level_b_cloud()
    assert all(_pack21(v)[0] for v in np.floor(pts / pc.VOXEL_A)) and len(okicp.voxel_downsample(pts, pc.VOXEL_A)) == pc.RANGE_N
    assert not any(_pack21(v)[0] for v in np.floor(pts / pc.LEVEL_B_VOXEL))
    r = np.sqrt((pts * pts).sum(axis=1))
    assert np.all((r > 149.0) & (r < pc.FAR_RANGE / 2))
