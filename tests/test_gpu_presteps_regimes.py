"""The chained pre-steps on the GPU (kicp_pre.hpp k_frame_*, k_downsample_*, k_scan_blocks; kicp_pre.hip pre_frame_chain) in
the regimes tests/test_gpu_presteps.py never provably enters: second-level launches whose workgroups walk several table tiles or
find none, more point tiles than table tiles under a right guess and the reverse, tables of at most 512 buckets (the small path of
replay_tile) at either level, survivor counts on a power-of-two bracket edge with the guess on either side of it, a hopeless guess
(every claim gives up), range errors inside the chain - the voxel whose key aliases an in-range neighbour's, the second level
alone, coordinates that are not finite - and the handle's life after them, grids beyond 4 096 workgroups (the separate scan
kernel, several turns of its loop), and one handle whose capacity grows between frames.

The cases and their premises: tests/prestep_cases.py, proved on the CPU in tests/test_prestep_cases.py.  Every case is held to the
oracle (buffer 0 to the 1e-11 of tests/test_gpu_presteps.py, buffers 1 and 2 exactly: a downsample only selects input points), to
the reference build where it is there, to a second handle that runs the unfused chain (bit for bit: three buffers, the counts, the
returned frame), and to the read-only counters of kicp_pre_get_option, which prove that the regime was entered - a moved threshold
fails here instead of silently uncovering the path."""
import functools

import numpy as np
import pytest

import kinematic_icp_amd as K
import prestep_cases as pc
from oracle import rkicp

pytestmark = pytest.mark.gpu
COUNTERS = ("fused_frames", "guess_misses", "point_tiles", "l1_tiles", "l2_workgroups", "l2_tiles", "scan_launches")
REF_BUILD_LIMIT = 40000  # frames up to this size are also held to the reference build's VoxelDownsample


def counters(pre):
    return {k: int(pre.get_option(k)) for k in COUNTERS}


def plain_handle():
    pre = K.PreSteps()
    pre.set_option("fused", 0)
    return pre


def run(pre, case, guess=True):
    """one Frame call -> (counts, returned frame, buffer 0, 1, 2).  The output buffers are filled with NaN first (buffer 3 is the
    frame's buffer 1: the two take turns): memory that still holds an earlier frame's points - the same cloud's, from this handle or
    from a freed one - would hide a store that was never made."""
    poison = np.full((case.n_in, 3), np.nan)
    for b in (0, 2, 3):
        pre.upload(b, poison)
    if guess and case.guess is not None:
        pre.set_option("guess", case.guess)
    counts, frame = pre.Frame(case.build(), None, pc.IDENT, pc.IDENT, case.max_range, case.min_range, 0, case.voxel_a, case.voxel_b)
    assert pre.last_status == K.KICP_OK
    return counts, frame, pre.download(0), pre.download(1), pre.download(2)


def assert_same(got, want):
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        np.testing.assert_array_equal(a, b)


def assert_oracle(got, case):
    counts, frame, b0, b1, b2 = got
    o0, o1, o2 = pc.oracle_chain(case)
    assert counts == [len(o0), len(o1), len(o2)]
    if hasattr(case, "counts"):
        assert counts == case.counts
    np.testing.assert_array_equal(frame, b0)
    np.testing.assert_allclose(b0, o0, rtol=0, atol=1e-11)
    np.testing.assert_array_equal(b1, o1)
    np.testing.assert_array_equal(b2, o2)
    if rkicp.available() and case.n_in <= REF_BUILD_LIMIT and counts[0]:
        np.testing.assert_array_equal(b1, rkicp.voxel_downsample(b0, case.voxel_a))
        np.testing.assert_array_equal(b2, rkicp.voxel_downsample(b1, case.voxel_b))


def both(fused, plain, case):
    """the case through the fused and the unfused handle: equal to each other and to the oracle; returns the fused handle's
    counters before and after"""
    before = counters(fused)
    got = run(fused, case)
    after = counters(fused)
    assert_same(got, run(plain, case, guess=False))
    assert_oracle(got, case)
    assert counters(plain)["fused_frames"] == 0
    return before, after


def assert_fused(before, after, case, hit=True):
    """the frame went through the five launches, with the tiles the case implies; the guess was right / wrong"""
    assert after["fused_frames"] == before["fused_frames"] + 1
    assert after["guess_misses"] == before["guess_misses"] + (0 if hit else 1)
    assert hit == case.hit
    assert (after["point_tiles"], after["l1_tiles"], after["l2_tiles"]) == (case.point_tiles, case.l1_tiles, case.l2_tiles)
    assert after["scan_launches"] == before["scan_launches"]  # (frame-sized grids add the counts up themselves)


@functools.lru_cache(maxsize=None)
def fresh(case):
    """what a handle that has seen nothing gives for the case (computed once, shared, read-only)"""
    got = run(K.PreSteps(), case, guess=False)
    for a in got[1:]:
        a.setflags(write=False)
    return got


def test_second_level_walks_several_tiles_per_workgroup():
    """k_frame_l2_replay / k_frame_l2_gather size their grid from the PREVIOUS frame's second table: behind a 300-point frame 32
    workgroups walk the 64 tiles of a table of 6 000 level-1 survivors - the second turn of their loops, the loads that are not
    the workgroup's prefetched first tile."""
    fused, plain = K.PreSteps(), plain_handle()
    before, after = both(fused, plain, pc.ORDINARY)
    assert_fused(before, after, pc.ORDINARY)
    case = pc.L2_SEVERAL_TILES
    before, after = both(fused, plain, case)
    assert_fused(before, after, case)
    assert after["l2_workgroups"] == 32 == pc.l2_workgroups(case.n_in, pc.ORDINARY.n1)
    assert after["l2_tiles"] >= 64 and case.n1 > 4096


@pytest.mark.parametrize("case", pc.TILE_CASES, ids=repr)
def test_workgroups_without_a_tile_and_point_tiles_against_table_tiles(case):
    """A fresh handle's second-level launches are several hundred workgroups wide: for the one tile of a frame that lies in one
    voxel, for none where the crop leaves nothing.  157 point tiles against the 8 table tiles of a rightly guessed crop that keeps
    1 000 points (k_frame_l1_replay: grid > tiles_spec), and against 512 where nothing is cropped."""
    fused, plain = K.PreSteps(), plain_handle()
    before, after = both(fused, plain, case)
    assert_fused(before, after, case)
    assert after["l2_workgroups"] == pc.l2_workgroups(case.n_in, None) >= 256 > after["l2_tiles"]
    assert after["point_tiles"] == 157 and after["l1_tiles"] == (8 if case is pc.FEW_SURVIVE else 512)


@pytest.mark.parametrize("case", pc.SMALL_CASES + [pc.SMALL_B], ids=repr)
def test_small_and_window_tables_through_the_frame(case):
    """Tables of at most 512 buckets take replay_tile's global path, 1 024 buckets (257 points) the LDS window: at both levels, and
    with table A through the window while table B is small."""
    fused, plain = K.PreSteps(), plain_handle()
    before, after = both(fused, plain, case)
    assert_fused(before, after, case)
    assert (pc.buckets(case.n1) <= pc.SMALL_TABLE_BUCKETS) == (case.n1 <= 256)


@pytest.mark.parametrize("n0", pc.SMALL_COUNTS)
def test_small_and_window_tables_through_the_downsample(n0):
    case = pc.SMALL_CASES[pc.SMALL_COUNTS.index(n0)]
    o0, o1, o2 = pc.oracle_chain(case)
    pre = K.PreSteps()
    pre.upload(0, o0)
    for b in (1, 2):  # (as run(): nothing an earlier test left in memory stands in for a store)
        pre.upload(b, np.full((n0, 3), np.nan))
    assert pre.VoxelDownsample(0, case.voxel_a, 1) == len(o1) == n0 and pre.last_status == K.KICP_OK
    assert pre.VoxelDownsample(1, case.voxel_b, 2) == len(o2)
    np.testing.assert_array_equal(pre.download(1), o1)
    np.testing.assert_array_equal(pre.download(2), o2)
    if rkicp.available():
        np.testing.assert_array_equal(pre.download(1), rkicp.voxel_downsample(o0, case.voxel_a))
        np.testing.assert_array_equal(pre.download(2), rkicp.voxel_downsample(o1, case.voxel_b))
    assert counters(pre)["scan_launches"] == 0


@pytest.mark.parametrize("case", pc.EDGE_CASES, ids=repr)
def test_counts_on_a_bracket_edge_with_the_guess_on_either_side(case):
    """2^k points keep 2^(k+1) buckets, one more takes 2^(k+2): the device's test of the guess (expected_mask(n0) == spec_mask) and
    the second table's size turn on that edge.  Count and guess on the same side: fused, no miss; on different sides: one miss and
    the unfused downsamples.  The same buffers either way."""
    fused, plain = K.PreSteps(), plain_handle()
    before, after = both(fused, plain, case)
    assert_fused(before, after, case, hit=case.n0 == case.guess)


def test_a_hopeless_guess_then_a_right_one():
    """A table of two buckets for 20 000 voxels: every claim of k_frame_pre gives up after kClaimProbeLimit probes and says so; the
    frame is finished by the unfused downsamples, the tables are cleaned, and the next frame - rightly guessed - is fused."""
    fused, plain = K.PreSteps(), plain_handle()
    before, after = both(fused, plain, pc.HOPELESS)
    assert_fused(before, after, pc.HOPELESS, hit=False)
    before, after = both(fused, plain, pc.HOPELESS_THEN_RIGHT)
    assert_fused(before, after, pc.HOPELESS_THEN_RIGHT)
    assert after["l2_workgroups"] == 32 < after["l2_tiles"] == 256  # (eight turns of the second level's tile loops)


# ---- range errors ----------------------------------------------------------------------------------------------------------------
def frame_of(pre, pts, voxel_b=pc.VOXEL_B):
    return pre.Frame(pts, None, pc.IDENT, pc.IDENT, pc.FAR_RANGE, pc.MIN_RANGE, 0, pc.VOXEL_A, voxel_b)


def downsample_of(pre, pts, voxel_b=pc.VOXEL_B):
    pre.upload(0, pts)
    n1 = pre.VoxelDownsample(0, pc.VOXEL_A, 1)
    return [len(pts), n1, pre.VoxelDownsample(1, voxel_b, 2)], None


ENTRIES = (("VoxelDownsample", K.PreSteps, downsample_of), ("fused Frame", K.PreSteps, frame_of), ("unfused Frame", plain_handle, frame_of))


def assert_range_error_then_life_goes_on(pts, voxel_b=pc.VOXEL_B, entries=ENTRIES):
    """every entry answers KICP_ERR_CAPACITY, once: the same handle then takes an ordinary frame and gives a fresh handle's result"""
    for name, make, entry in entries:
        pre = make()
        before = counters(pre)
        with pytest.raises(K.KicpError) as e:
            entry(pre, pts, voxel_b)
        assert e.value.code == K.KICP_ERR_CAPACITY, name
        after = counters(pre)
        assert after["fused_frames"] - before["fused_frames"] == (1 if name == "fused Frame" else 0), name
        assert after["guess_misses"] == 0, name  # (the error came out of the five launches, not out of the unfused tail)
        assert_same(run(pre, pc.ORDINARY), fresh(pc.ORDINARY))  # (run: the call returns KICP_OK - nothing is reported twice)
        later = counters(pre)  # ... through the five launches and the tables the failed call left behind, where the handle fuses
        assert later["fused_frames"] - after["fused_frames"] == (0 if name == "unfused Frame" else 1) and later["guess_misses"] == 0, name


@pytest.mark.parametrize("axis,sign,k", pc.TWIN_CASES)
def test_a_voxel_whose_key_aliases_its_neighbours_is_out_of_range(axis, sign, k):
    """pack_voxel21 masks to 21 bits: the voxel 2^21 beyond an in-range one carries that one's key.  Directly behind a point of
    that neighbour, inside one wave (k + 1 = 11), the run test of claim_voxel took it for a duplicate and swallowed it - KICP_OK,
    one survivor too few -; first in its wave (k + 1 = 64) it always reached the range test."""
    assert_range_error_then_life_goes_on(pc.twin_cloud(axis, sign, k))


def test_the_second_level_alone_leaves_the_range():
    """voxel_b far smaller than voxel_a (the API allows it): 150 m are 300 voxels of 0.5 m and 1.5e6 of 1e-4 m"""
    pts = pc.level_b_cloud()
    pre = K.PreSteps()
    pre.upload(0, pts)
    assert pre.VoxelDownsample(0, pc.VOXEL_A, 1) == pc.RANGE_N  # (the first level is in range)
    assert_range_error_then_life_goes_on(pts, voxel_b=pc.LEVEL_B_VOXEL)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("value", pc.NONFINITE, ids=str)
def test_a_coordinate_that_is_not_finite_is_out_of_range(value, axis):
    """Preprocess drops such points at the range crop; kicp_pre_upload + kicp_pre_voxel_downsample take any doubles.  The device
    table cannot express the reference's INT_MIN voxel: the documented answer is the range error (include/kicp.h)."""
    assert_range_error_then_life_goes_on(pc.nonfinite_cloud(value, axis, 10), entries=ENTRIES[:1])


# ---- beyond 4 096 workgroups -----------------------------------------------------------------------------------------------------
def test_the_downsample_at_the_edge_of_the_separate_scan():
    """524 288 points: 1 048 576 buckets, 4 096 workgroups, every workgroup adds the counts before it up itself; one point more:
    8 192 workgroups, k_scan_blocks (eight turns of its loop, a carry between them) and the `raw == 0` side of block_offset."""
    pts = pc.BIG.build()
    pre = K.PreSteps()
    for n, scans in ((pc.VD_LAST_FUSED, 0), (pc.VD_FIRST_SCANNED, 1)):
        pre.upload(0, pts[:n])
        pre.upload(1, np.full((n, 3), np.nan))  # (the first size's survivors are nearly the second's: none may stand in for a store)
        before = counters(pre)["scan_launches"]
        want = pc.oracle_downsample_of_big_prefix(n)
        assert pre.VoxelDownsample(0, pc.VOXEL_A, 1) == len(want) and pre.last_status == K.KICP_OK
        assert counters(pre)["scan_launches"] == before + scans
        np.testing.assert_array_equal(pre.download(1), want)


def test_preprocess_beyond_4096_point_tiles():
    big = pc.BIG
    o0 = pc.oracle_chain(big)[0]
    pre = K.PreSteps()
    pre.upload(0, np.full((big.n_in, 3), np.nan))
    assert pre.Preprocess(big.build(), None, pc.IDENT, pc.IDENT, big.max_range, big.min_range, 0, dst=0) == len(o0)
    assert counters(pre)["scan_launches"] == 1
    np.testing.assert_allclose(pre.download(0), o0, rtol=0, atol=1e-11)


def test_the_frame_beyond_4096_point_tiles_is_not_fused():
    """pre_frame_chain refuses to fuse: preprocess, scan, compact, and a scan in front of either gather - three scan launches"""
    fused, plain = K.PreSteps(), plain_handle()
    before, after = both(fused, plain, pc.BIG)
    assert after["fused_frames"] == before["fused_frames"] == 0 and after["guess_misses"] == 0
    assert after["scan_launches"] == before["scan_launches"] + 3 and counters(plain)["scan_launches"] == 3


def test_one_handle_whose_capacity_grows_between_frames():
    """pre_ensure enlarges table_slots, which moves min_index, order and home_at inside the tables' buffers: 300, 40 000, 300,
    1 048 577 and 300 points through one handle, each frame what a fresh handle gives."""
    pre = K.PreSteps()
    sequence = (pc.ORDINARY, pc.GROWTH_MIDDLE, pc.ORDINARY, pc.BIG, pc.ORDINARY)
    assert [c.n_in for c in sequence] == [300, 40000, 300, 1048577, 300]
    for case in sequence:
        got = run(pre, case)
        assert_same(got, fresh(case))
        assert_oracle(got, case)
    c = counters(pre)
    assert c["fused_frames"] == 4 and c["guess_misses"] == 0 and c["scan_launches"] == 3
