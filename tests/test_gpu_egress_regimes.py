"""The clouds' way back to the host on the GPU (kicp_pre_egress.hpp k_push_frame / k_push_frame_f32 / k_narrow_f32, kicp_pre_egress.hip
follow_pushed_pieces / egress_settle / kicp_pre_download_finish, kicp_map_pc.hpp k_pc_records, kicp_map_cloud.hip kicp_map_pointcloud_f32)
in the regimes tests/test_gpu_egress.py and tests/test_gpu_presteps_regimes.py never provably enter: frames that end on, just
before and just behind a piece boundary, all eight pieces full, no survivor, one to four records, a piece longer than one sweep
of the grid; one handle whose piece size shrinks and whose landing area grows, with stale flags behind it, an uncollected frame, a
refused collection, a handle destroyed with a push out; other grid widths and the DMA route (in child processes); the keypoints'
records behind a missed guess; the narrowing kernel's second turn; map buckets deeper than an LDS round, maps of one to five
points, sparse tables and the piece rule's edges.

The cases and their premises: tests/egress_cases.py, proved on the CPU in tests/test_egress_cases.py.  The reference is always the
fp64 path's own bytes narrowed by numpy (egress_ref.narrow), compared as words - there is no tolerance but buffer 0's 1e-11 to the
oracle - and every test asserts from the read-only counters ("push_launches" / "push_pieces" of kicp_pre_get_option, "guess_misses",
"record_pieces" of kicp_map_update_counts) that it took the path it is named after."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import egress_cases as ec
import egress_ref as E
import kinematic_icp_amd as K
import prestep_cases as pc
from mapdev_ref import Oracles
from test_egress import pointcloud_f32

pytestmark = pytest.mark.gpu
SENTINEL32 = 0xDEADBEEF
_dp = C.POINTER(C.c_double)


def dptr(a):
    return a.ctypes.data_as(_dp)


def push_counters(pre):
    return int(pre.get_option("push_launches")), int(pre.get_option("push_pieces"))


def landing_array(n_in, f32):
    """the caller's array, filled with a sentinel: 0xDEADBEEF words for records, NaN for doubles"""
    return np.full((n_in, 3), SENTINEL32, dtype=np.uint32) if f32 else np.full((n_in, 3), np.nan)


def poison(pre, case):
    """as run() of tests/test_gpu_presteps_regimes.py: no point an earlier frame left in memory stands in for a store"""
    nan = np.full((case.n_in, 3), np.nan)
    for b in (0, 2, 3):
        pre.upload(b, nan)


def start_frame(pre, case, f32, out, guess=True, poisoned=True):
    """kicp_pre_frame / kicp_pre_frame_f32 straight through the C entry, the frame landing in `out`; nothing is collected"""
    if poisoned:
        poison(pre, case)
    if guess and case.guess is not None:
        pre.set_option("guess", case.guess)
    pts = np.ascontiguousarray(case.build())
    ident = np.ascontiguousarray(pc.IDENT)
    counts = (C.c_size_t * 3)()
    entry = K.lib().kicp_pre_frame_f32 if f32 else K.lib().kicp_pre_frame
    rc = entry(pre._h, dptr(pts), case.n_in, None, 0, dptr(ident), dptr(ident), case.max_range, case.min_range, 0, case.voxel_a, case.voxel_b,
               out.ctypes.data if f32 else dptr(out), case.n_in, counts)
    assert rc == K.KICP_OK
    return [int(c) for c in counts]


def collect(pre, out, f32):
    """kicp_pre_download_finish as the wrapper calls it: the doubles with the call's own pointer, the records with NULL"""
    n = C.c_size_t()
    rc = K.lib().kicp_pre_download_finish(pre._h, 0, None if f32 else dptr(out), 0 if f32 else len(out), C.byref(n))
    return rc, n.value


def assert_landed(out, n0, want_b0, f32):
    """the first n0 records are the frame - buffer 0's doubles, narrowed for records -, everything behind them is the sentinel"""
    if f32:
        assert np.array_equal(out[:n0], E.narrow(want_b0))
        assert np.all(out[n0:] == SENTINEL32)
    else:
        assert np.array_equal(out[:n0].view(np.uint64), np.ascontiguousarray(want_b0).view(np.uint64))
        assert np.all(np.isnan(out[n0:]))


def check_push(pre, case, f32, pushed=True, sentinel=True):
    """one frame through the handle, collected: counts, buffer 0 against the oracle, the landed frame against buffer 0, the
    sentinel behind it, and the counters - one launch, and the worker followed the flags the piece rule predicts"""
    rec = 12 if f32 else 24
    before = push_counters(pre)
    out = landing_array(case.n_in, f32)
    counts = start_frame(pre, case, f32, out)
    rc, n = collect(pre, out, f32)
    after = push_counters(pre)
    assert rc == K.KICP_OK and n == counts[0] and counts == case.counts
    b0, o0 = pre.download(0), pc.oracle_chain(case)[0]
    np.testing.assert_allclose(b0, o0, rtol=0, atol=1e-11)
    assert_landed(out if sentinel else out[:counts[0]], counts[0], b0, f32)
    followed = ec.frame_pieces_followed(case.n0, case.n_in, rec)
    assert (after[0] - before[0], after[1] - before[1]) == ((1, followed) if pushed else (0, 0))
    return out[:counts[0]]


@functools.lru_cache(maxsize=None)
def fresh(case, f32):
    """what a handle that has seen nothing returns for the case (computed once, shared, read-only)"""
    out = check_push(K.PreSteps(), case, f32)
    out.setflags(write=False)
    return out


# ---- the frame's pieces ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stale", [False, True], ids=["fresh_handle", "after_40000"])
@pytest.mark.parametrize("case", ec.PUSH_CASES, ids=repr)
def test_a_frame_case_through_both_entries(case, stale):
    """Every case as doubles and as records (the case is named after the record size whose pieces it pins; the other entry's
    pieces follow from the same rule), on a fresh handle and behind a 40 000-point frame whose flags - lengths of 122 880 bytes,
    above the case's piece size - are still in host memory: only the sequence tag tells them from the new ones."""
    for f32 in (False, True):
        pre = K.PreSteps()
        if stale:
            counts, frame = pre.Frame(ec.STALE_MAKER.build(), None, pc.IDENT, pc.IDENT, pc.MAX_RANGE, pc.MIN_RANGE, 0, pc.VOXEL_A, pc.VOXEL_B)
            assert counts[0] == len(frame) == ec.STALE_MAKER.n0 and push_counters(pre) == (1, 6)
        got = check_push(pre, case, f32)
        if f32 == (case.rec_bytes == 12):  # the pieces the case's name promises (tests/test_egress_cases.py: the rule gives them)
            assert ec.frame_pieces(case.n0, case.n_in, 12 if f32 else 24) == case.pieces
            assert push_counters(pre)[1] - (6 if stale else 0) == case.followed
        assert np.array_equal(got, fresh(case, f32))


# ---- one handle over time --------------------------------------------------------------------------------------------------------
def test_one_handle_whose_piece_size_shrinks_and_whose_entries_alternate():
    """300, 44 000, 1 365, 4 096 and 300 input points through one handle, doubles and records in turn, a frame nobody wants back
    in between: every frame what a fresh handle returns, every launch's pieces followed."""
    pre = K.PreSteps()
    assert [c.n_in for c in ec.SEQUENCE] == [300, 44000, 1365, 4096, 300]
    for k, case in enumerate(ec.SEQUENCE):
        f32 = k % 2 == 1
        assert np.array_equal(check_push(pre, case, f32), fresh(case, f32))
        if k == 2:  # want_frame=False: nothing is pushed, the counters stand still, the keypoints' records are there
            before = push_counters(pre)
            other = ec.PUSH_CASES[13]
            counts, none = pre.FrameF32(other.build(), None, pc.IDENT, pc.IDENT, pc.MAX_RANGE, pc.MIN_RANGE, 0, pc.VOXEL_A, pc.VOXEL_B, want_frame=False)
            assert counts == other.counts and none is None and push_counters(pre) == before
            assert np.array_equal(pre.download_f32(2).view(np.uint32), E.narrow(pc.oracle_chain(other)[2]))
    assert push_counters(pre)[0] == 5


def test_the_landing_area_grows_between_frames():
    """landing_reserve: a 300-point frame leaves room for 1 059 376 bytes; 50 000 points as doubles need 1 200 000 - the pinned
    area is reallocated between two pushes, and the next, small frame lands in the new one"""
    pre = K.PreSteps()
    first, grows = ec.LANDING_FIRST, ec.LANDING_GROWS
    assert first.n_in * 24 * 3 // 2 + (1 << 20) < grows.n_in * 24
    for case, f32 in ((first, False), (grows, False), (ec.PUSH_CASES[2], True), (first, True)):
        assert np.array_equal(check_push(pre, case, f32), fresh(case, f32))


def test_a_frame_nobody_collected_is_finished_by_the_next_call():
    """Straight through the C entry: a frame is started and never collected; the next call (egress_settle) joins its copy worker
    before it queues its own push, so the first array is complete when the second call returns.  (Both frames are small: the first
    push has long ended when the second call refills buffer 0.)  Collecting buffer 0 twice is an error."""
    pre = K.PreSteps()
    a, b = ec.PUSH_CASES[3], ec.PUSH_CASES[2]
    for f32 in (False, True):
        before = push_counters(pre)
        out_a, out_b = landing_array(a.n_in, f32), landing_array(b.n_in, f32)
        counts_a = start_frame(pre, a, f32, out_a)
        counts_b = start_frame(pre, b, f32, out_b, poisoned=False)  # (no upload into buffer 0 of this test's own in between)
        assert counts_a == a.counts and counts_b == b.counts
        assert np.array_equal(out_a[:a.n0], fresh(a, f32))  # (before anything is collected)
        assert np.all(out_a[a.n0:] == SENTINEL32) if f32 else np.all(np.isnan(out_a[a.n0:]))
        assert collect(pre, out_b, f32) == (K.KICP_OK, b.n0)
        assert_landed(out_b, b.n0, pre.download(0), f32)
        assert np.array_equal(out_b[:b.n0], fresh(b, f32))
        rec = 12 if f32 else 24
        after = push_counters(pre)
        assert after[0] - before[0] == 2
        assert after[1] - before[1] == ec.frame_pieces_followed(a.n0, a.n_in, rec) + ec.frame_pieces_followed(b.n0, b.n_in, rec)
        assert collect(pre, out_b, f32)[0] == K.KICP_ERR_ARG  # no download of buffer 0 is in flight any more
    assert np.array_equal(check_push(pre, a, False), fresh(a, False))


def test_records_are_refused_to_another_pointer():
    """kicp_pre_download_finish of a FLOAT32 frame with a pointer that is not the call's own: the records went to the call's array
    (complete by then: the worker was joined), nothing can be copied into doubles - KICP_ERR_ARG, and the handle goes on"""
    pre = K.PreSteps()
    case = ec.PUSH_CASES[12]
    out, other = landing_array(case.n_in, True), np.full((case.n_in, 3), np.nan)
    assert start_frame(pre, case, True, out) == case.counts and case.n0 > 0
    n = C.c_size_t()
    assert K.lib().kicp_pre_download_finish(pre._h, 0, dptr(other), case.n_in, C.byref(n)) == K.KICP_ERR_ARG
    assert np.all(np.isnan(other))
    assert_landed(out, case.n0, pre.download(0), True)
    assert collect(pre, out, True)[0] == K.KICP_ERR_ARG  # (the refused collection ended the download)
    for f32 in (True, False):
        assert np.array_equal(check_push(pre, case, f32), fresh(case, f32))


def test_a_handle_destroyed_with_a_push_out():
    """kicp_pre_destroy joins the copy worker and drains the download stream: the array - alive until after the handle has gone -
    holds the whole frame"""
    case = ec.PUSH_CASES[16]
    for f32 in (False, True):
        pre = K.PreSteps()
        out = landing_array(case.n_in, f32)
        assert start_frame(pre, case, f32, out) == case.counts
        del pre
        assert np.array_equal(out[:case.n0], fresh(case, f32))
        assert np.all(out[case.n0:] == SENTINEL32) if f32 else np.all(np.isnan(out[case.n0:]))


# ---- the keypoints' records ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.KEYPOINT_CASES, ids=repr)
def test_the_keypoints_records_with_the_guess_right_and_wrong(case):
    """Behind a FLOAT32 frame whose guess was right the records of buffer 2 are in host memory (k_frame_src_host); behind a miss the
    chain took the unfused tail, nothing is on the host and k_narrow_f32 narrows the buffer.  Either way they are the doubles
    narrowed, and the doubles are the oracle's.  The same behind an fp64 frame (the host copy holds doubles: narrowed in HBM)."""
    o2 = pc.oracle_chain(case)[2]
    for f32 in (True, False):
        pre = K.PreSteps()
        check_push(pre, case, f32)  # (the frame itself, its pieces and buffer 0, as every frame of this module)
        assert len(o2) == case.n2
        assert int(pre.get_option("fused_frames")) == 1 and int(pre.get_option("guess_misses")) == (0 if case.hit else 1)
        records, doubles = pre.download_f32(2), pre.download(2)
        assert records.shape == (case.n2, 3) and np.array_equal(doubles, o2)
        assert np.array_equal(records.view(np.uint32), E.narrow(doubles))
        assert np.array_equal(pre.download_f32(1).view(np.uint32), E.narrow(pc.oracle_chain(case)[1]))


@pytest.mark.parametrize("n", ec.NARROW_SIZES)
def test_the_narrowing_kernel_at_the_edge_of_its_grid(n):
    """k_narrow_f32: 1 024 workgroups of 256 lanes; 87 381 points are the last that one turn of its loop narrows"""
    pts = ec.narrow_points(n)
    pre = K.PreSteps()
    pre.upload(0, pts)
    assert np.array_equal(pre.download_f32(0).view(np.uint32), E.narrow(pts))


def test_the_narrowing_scratch_grows_and_is_reused():
    pre = K.PreSteps()
    for n in (ec.NARROW_GROW, ec.NARROW_REUSE, ec.NARROW_SIZES[2]):
        pts = ec.narrow_points(n, seed=141)
        pre.upload(0, pts)
        got = pre.download_f32(0)
        assert got.shape == (n, 3) and np.array_equal(got.view(np.uint32), E.narrow(pts))


# ---- other grid widths, in child processes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("wgs,lines", [("1", 8), ("3", 8), ("0", 10)])
def test_the_push_with_another_grid_width(wgs, lines):
    """KICP_PRE_PUSH_WGS is read once per process: tests/egress_grid_width.py runs the exact-boundary and the all-full cases through
    both entries in a process of its own - one workgroup (every piece's ticket_done is 1 further), three (a sweep of 12 288 bytes:
    the all-full pieces in exactly one), and 0: the DMA engine moves the doubles behind chain.ready, in pieces from 1 MiB on"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "egress_grid_width.py")
    run = subprocess.run([sys.executable, script], env=dict(os.environ, KICP_PRE_PUSH_WGS=wgs), timeout=120, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.splitlines()
    assert len(out) == lines and all(line.startswith("ok ") for line in out), run.stdout


# ---- the map's records -----------------------------------------------------------------------------------------------------------
def rows_sorted(a):
    return a[np.lexsort(a.T[::-1])]


def driven(scene):
    """the scene on a map with a device and on the oracles, in lock step; the last call's update_counts before and after"""
    m, o = K.VoxelHashMap(scene.voxel, scene.max_distance, scene.cap, device=0), Oracles(scene.voxel, scene.max_distance, scene.cap)
    before = None
    for k, (name, *args) in enumerate(scene.calls):
        if k == len(scene.calls) - 1:
            before = m.update_counts()
        for x in (m, o):
            getattr(x, name)(*args)
    assert K.lib().kicp_map_last_update_on_device(m._h) == 1
    return m, o, before, m.update_counts()


def read_records(m, ref, cap=None):
    """kicp_map_pointcloud_f32 with room for `cap` records: the first records of Pointcloud() narrowed, the sentinel untouched
    (the array holds no more than cap), and the device announced - and the host copied - exactly the pieces the rule predicts"""
    before = m.update_counts()["record_pieces"]
    rc, total, out = pointcloud_f32(m, cap)
    want = len(ref) if cap is None else min(cap, len(ref))
    assert rc == K.KICP_OK and total == len(ref)
    assert np.array_equal(out[:want], ref[:want]) and np.all(out[want:] == SENTINEL32)
    assert m.update_counts()["record_pieces"] - before == ec.map_pieces(want)
    return out


def check_scene(scene, extra_caps=()):
    """extra_caps: more sizes to read with, or a function of the map's fp64 cloud that gives them"""
    m, o, before, after = driven(scene)
    cloud = m.Pointcloud()
    ref = E.narrow(cloud)
    if callable(extra_caps):
        extra_caps = extra_caps(cloud)
    assert len(ref) == o.num_points() == len(ec.oracle_map_cloud(scene))
    full = read_records(m, ref)
    assert np.array_equal(rows_sorted(full), rows_sorted(E.narrow(o.buckets())))
    for cap in tuple(scene.caps) + tuple(extra_caps):
        read_records(m, ref, cap)
    assert np.array_equal(m.PointcloudF32().view(np.uint32), ref)
    assert K.lib().kicp_map_last_update_on_device(m._h) == 1 and m.update_counts()["host_updates"] == 0
    return m, ref, before, after


def test_a_bucket_deeper_than_an_lds_round():
    """cap 5 000, one voxel of 4 500 points: one lane's run spans three rounds of 2 048 records (k0 > 0 of the per-lane window); read
    whole, and with room that ends 2 047, 2 048, 2 049 and 4 100 records into the run"""
    scene = ec.deep_bucket()

    def cuts(cloud):
        deep = np.flatnonzero((np.floor(cloud / scene.voxel) == np.array(ec.DEEP_VOXEL)).all(axis=1))
        assert len(deep) == ec.DEEP_POINTS and deep[-1] - deep[0] == ec.DEEP_POINTS - 1  # one run
        return [int(deep[0]) + cut for cut in ec.DEEP_CUTS]

    check_scene(scene, extra_caps=cuts)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_a_map_of_a_few_points_on_the_device_path(k):
    """3 to 15 words in the only block that holds any: one record is less than one 16-byte unit (u0 >= u1), two to five are units
    and a tail of single words"""
    m, ref, _, _ = check_scene(ec.few_points(k), extra_caps=range(1, k))
    assert len(ref) == k == m.num_points()


def test_a_sparse_table():
    """a few hundred points in a table that held 40 000: most 256-slot blocks hold nothing - the search for the first block past lo,
    blocks skipped between lo and hi - read whole and in pieces of 1 024 that begin anywhere"""
    m, ref, before, after = check_scene(ec.sparse(), extra_caps=(1, 4, 100, 257))
    assert 150 < len(ref) < 700
    assert after["rehashes"] == before["rehashes"]  # (the pruning update kept the table: sized for the 40 000)


def test_the_piece_rules_edges_and_two_grid_widths_on_one_map():
    """4 096 records: four pieces of the 1 024-record minimum; 4 097: three of 2 048; 262 144: four of 65 536; 262 145: a fifth piece,
    the second ticket round of slot 0; then a small read and the whole map, whose launches differ in width - the slots' tickets are
    cumulative across all of them"""
    scene = ec.piece_edges()
    m, ref, _, _ = check_scene(scene)
    assert len(ref) >= 262145 and tuple(scene.caps) == (4096, 4097, 262144, 262145)
    for cap in (5, None, 4096, len(ref) - 3):
        read_records(m, ref, cap)
