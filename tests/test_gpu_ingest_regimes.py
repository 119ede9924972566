"""The PointCloud2 ingest on the GPU (kicp_pre_ingest.hpp k_ingest, kicp_pre_ingest.hip ingest_run) in the regimes tests/test_ingest.py never
enters: records longer than the 128 bytes that go through LDS (and 127, 128, 129), a point_step so long that every launch is one
workgroup, the one-term neighbours of the `aligned` predicate, negative stamps, the nanosecond rule's boundary values and clouds that
mix converting and non-converting stamps, full-range UINT32, extrema at tile and piece edges, in a one-record tail piece and in the
tiles a look-ahead launch visits on a later round, sizes on the tile and piece edges, fields that end at point_step, one handle used
down and up in size across layouts - and what consumes the result: Preprocess and the chained Frame on raw negative / mixed stamps
and on clouds full of NaN, infinite and (0, 0, 0) points.  The cases and their premises: tests/ingest_cases.py, proved on the CPU
in tests/test_ingest_cases.py.  Every case asserts from the read-only counters of kicp_pre_get_option ("ingest_*" / "ahead_*") that
it ran in the regime it is named after, so that a moved threshold fails here instead of silently uncovering the path."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import ingest_cases as ic
from checkers import okicp

pytestmark = pytest.mark.gpu
COUNTERS = ("launches", "workgroups", "aligned", "wide", "piece_records", "direct")


def counters(pre, prefix="ingest"):
    return {k: int(pre.get_option("%s_%s" % (prefix, k))) for k in COUNTERS}


def assert_regime(pre, case, prefix="ingest"):
    """the last decode of this slot went the way the case table says"""
    c = counters(pre, prefix)
    assert c["aligned"] == case.aligned and c["wide"] == case.wide, (case, c)
    assert c["piece_records"] == case.piece_records, (case, c)  # the rule of include/kicp.h, restated by ingest_cases.piece_records
    assert c["launches"] >= case.min_launches and c["launches"] == -(-case.n // c["piece_records"]), (case, c)
    assert c["direct"] in (0, 1)  # (no case needs either way of reaching the bytes)
    if prefix == "ingest":  # one workgroup per tile of the largest piece
        assert c["workgroups"] == -(-min(case.n, c["piece_records"]) // 256), (case, c)
    return c


def bits(values):
    return np.asarray(values, dtype=np.float64).view(np.uint64).tolist()


def assert_decoded(pre, m, lohi, want):
    """the handle's ingested cloud, stamps and extrema equal the oracle's (xyz, normalised stamps, (lo, hi)) bit for bit"""
    want_xyz, want_st, want_mm = want
    xyz, st = pre.ingested()
    ic.assert_same_cloud(xyz, want_xyz)
    assert bits(lohi) == bits(want_mm), (m.case, lohi, want_mm)
    if want_st is None:
        assert st is None
    else:
        np.testing.assert_array_equal(st, want_st)  # NaN == NaN positions too (constant stamps: 0/0)


@pytest.mark.parametrize("case", ic.DECODE_CASES, ids=repr)
def test_decode_equals_the_oracle(case):
    m = case.build()
    pre = K.PreSteps()
    lohi = pre.Ingest(*m.args)
    assert_regime(pre, case)
    assert_decoded(pre, m, lohi, okicp.ingest(*m.args))


def test_the_counters_describe_only_decodes_that_ran():
    pre = K.PreSteps()
    zero = dict.fromkeys(COUNTERS, 0)
    assert counters(pre) == zero and counters(pre, "ahead") == zero
    assert pre.get_option("ingest_nothing") == -1.0 and pre.get_option("ahead_") == -1.0
    case = ic.LAYOUT["s129_u32_last"]
    assert pre.Ingest(*case.args(b"", 0)) == (0.0, 0.0) and counters(pre) == zero  # (an empty message launches nothing)
    m = ic.POSE_CASE.build()
    pre.Ingest(*m.args)
    before = assert_regime(pre, ic.POSE_CASE)
    assert pre.Ingest(*case.args(b"", 0)) == (0.0, 0.0) and counters(pre) == before and counters(pre, "ahead") == zero


def test_one_handle_down_and_up_in_size_across_layouts():
    """The tickets are never reset and block_minmax keeps the keys of earlier, larger messages: the whole case list through ONE
    handle in a fixed shuffled order - sizes down and up, layouts and stamp types changing from message to message."""
    order = np.random.Generator(np.random.PCG64(5)).permutation(len(ic.DECODE_CASES))
    sizes = [ic.DECODE_CASES[k].n for k in order]
    assert any(a > 4 * b for a, b in zip(sizes, sizes[1:])) and any(b > 4 * a for a, b in zip(sizes, sizes[1:]))
    pre = K.PreSteps()
    for k in order:
        case = ic.DECODE_CASES[k]
        m = case.build()
        lohi = pre.Ingest(*m.args)
        assert_regime(pre, case)
        assert_decoded(pre, m, lohi, okicp.ingest(*m.args))
    assert pre.ahead_hits() == 0


def test_look_ahead_decodes_wide_unaligned_and_second_round_tiles():
    """IngestAhead + the chained Frame of the message before + Ingest: a wide layout, the layout whose 8-byte terms alone fail, and
    packed records whose extrema sit in tiles that the launch's workgroups reach on the second and third round of their tile loop.
    Each equals the plain sequence (cloud, extrema, every output of the chained pre-steps) and the oracle bit for bit."""
    rel, ext = ic.prestep_poses()
    msgs = [c.build() for c in ic.AHEAD_CASES]

    def chain(pre):
        counts, frame = pre.Frame(None, None, rel, ext, ic.MAX_RANGE, 1.0, True, ic.VOXEL_A, ic.VOXEL_B)
        return counts, frame, pre.download(1), pre.download(2)

    plain, ahead = K.PreSteps(), K.PreSteps()
    want = []
    for m in msgs:
        lohi = plain.Ingest(*m.args)
        want.append((lohi, plain.ingested(), chain(plain)))
    rounds = []
    for k, m in enumerate(msgs):
        hits = ahead.ahead_hits()
        lohi = ahead.Ingest(*m.args)
        assert ahead.ahead_hits() == hits + (1 if k else 0)  # (the opener is an ordinary message)
        if k:
            c = assert_regime(ahead, m.case, "ahead")
            tiles = -(-min(m.n, c["piece_records"]) // 256)  # of piece 0, the largest
            assert 1 <= c["workgroups"] <= tiles
            if tiles > c["workgroups"]:  # the extrema's tiles are visited on a later round of the tile loop
                for i in (m.imin, m.imax):
                    assert i < c["piece_records"] and i // 256 >= c["workgroups"], (m.case, c)
                    rounds.append(i // 256 // c["workgroups"])
        assert_decoded(ahead, m, lohi, okicp.ingest(*m.args))
        got_cloud = ahead.ingested()
        if k + 1 < len(msgs):
            ahead.IngestAhead(*msgs[k + 1].args)
        got = chain(ahead)  # (uploads and decodes message k + 1 behind its own kernels)
        assert bits(lohi) == bits(want[k][0])
        np.testing.assert_array_equal(got_cloud[0], want[k][1][0])
        np.testing.assert_array_equal(got_cloud[1], want[k][1][1])
        assert got[0] == want[k][2][0] and 0 < got[0][2] <= got[0][1] <= got[0][0] < m.n
        for a, b in zip(got[1:], want[k][2][1:]):
            np.testing.assert_array_equal(a, b)
    assert ahead.ahead_hits() == len(msgs) - 1 and plain.ahead_hits() == 0
    assert len(rounds) == 4 and min(rounds) >= 1 and max(rounds) >= 2
    assert counters(ahead, "ingest")["launches"] == 2 and counters(plain, "ahead")["launches"] == 0  # (only the opener went the plain way)


def test_sensor_pose_on_the_field_by_field_path():
    from kinematic_icp_amd import synthetic as syn
    case = ic.POSE_CASE
    m = case.build()
    T = syn.pose_mul(syn.planar_pose(0.3, -0.2, 0.4, 1.1), np.array([np.sin(0.1), 0, 0, np.cos(0.1), 0, 0, 0]))
    pre = K.PreSteps()
    lohi = pre.Ingest(*m.args, sensor_pose=T)
    c = assert_regime(pre, case)
    assert c["wide"] == 1 and c["aligned"] == 0 and c["launches"] == 2
    exp_xyz, exp_st, exp_mm = okicp.ingest(*m.args, sensor_pose_qt=T)
    xyz, st = pre.ingested()
    np.testing.assert_allclose(xyz, exp_xyz, rtol=0, atol=1e-12)  # (the tolerance of test_gpu_ingest_with_sensor_pose_and_errors)
    assert np.abs(xyz - okicp.ingest(*m.args)[0]).max() > 0.1  # (the pose is not trivial)
    assert bits(lohi) == bits(exp_mm)
    np.testing.assert_array_equal(st, exp_st)


def assert_same_buffers(a, b):
    for buf in (0, 1, 2):
        np.testing.assert_array_equal(a.download(buf), b.download(buf))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("deskew", [False, True])
@pytest.mark.parametrize("case", ic.STAMP_CONSUMER_CASES, ids=repr)
def test_consumers_of_raw_negative_and_mixed_stamps(case, deskew, fused):
    """The stamps stay in seconds on the device and are normalised where they are consumed (PreprocessParams::ts_normalise): fed
    from the ingested cloud, PreprocessIngested and the chained Frame give what the same calls give when fed the oracle's decoded
    host arrays, bit for bit, and the oracle's Preprocess to the 1e-11 of
    test_gpu_pipeline_from_raw_bytes_equals_pipeline_from_host_arrays, with equal counts."""
    rel, ext = ic.prestep_poses()
    m = case.build()
    xyz, st, _ = okicp.ingest(*m.args)
    a, b = K.PreSteps(), K.PreSteps()
    a.set_option("fused", fused), b.set_option("fused", fused)
    a.Ingest(*m.args)
    assert_regime(a, case)
    ref = okicp.se3_act(ext, okicp.preprocess(xyz, st, rel, ic.MAX_RANGE, ic.STAMP_CONSUMER_MIN_RANGE, deskew))
    na = a.PreprocessIngested(rel, ext, ic.MAX_RANGE, ic.STAMP_CONSUMER_MIN_RANGE, deskew, dst=0)
    nb = b.Preprocess(xyz, st, rel, ext, ic.MAX_RANGE, ic.STAMP_CONSUMER_MIN_RANGE, deskew, dst=0)
    assert na == nb == len(ref) and 0 < na < m.n
    np.testing.assert_array_equal(a.download(0), b.download(0))
    np.testing.assert_allclose(a.download(0), ref, rtol=0, atol=1e-11)
    ca, fa = a.Frame(None, None, rel, ext, ic.MAX_RANGE, ic.STAMP_CONSUMER_MIN_RANGE, deskew, ic.VOXEL_A, ic.VOXEL_B)
    cb, fb = b.Frame(xyz, st, rel, ext, ic.MAX_RANGE, ic.STAMP_CONSUMER_MIN_RANGE, deskew, ic.VOXEL_A, ic.VOXEL_B)
    assert ca == cb and ca[0] == len(ref) and 0 < ca[2] <= ca[1] <= ca[0]
    np.testing.assert_array_equal(fa, fb)
    np.testing.assert_allclose(fa, ref, rtol=0, atol=1e-11)
    assert_same_buffers(a, b)
    assert a.get_option("fused_frames") == fused and b.get_option("fused_frames") == fused


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("min_range", ic.INVALID_MIN_RANGES)
@pytest.mark.parametrize("deskew", [False, True])
def test_invalid_points_are_dropped_where_the_reference_drops_them(deskew, min_range, fused):
    """A fifth of the records are all-NaN, x = +inf, z = NaN only or (0, 0, 0), as in an organised cloud.  The reference drops NaN
    and infinite points at the range crop and keeps a zero point that deskewing has moved off the origin: survivor counts and
    points equal the oracle's through Ingest + PreprocessIngested / Frame and through Preprocess / Frame of host arrays, and both
    downsample counts equal VoxelDownsample of the oracle's survivors."""
    rel, ext = ic.prestep_poses()
    case = ic.INVALID_CASE
    m = case.build()
    xyz, st, _ = okicp.ingest(*m.args)
    ref = okicp.se3_act(ext, okicp.preprocess(xyz, st, rel, ic.MAX_RANGE, min_range, deskew))
    down_a = okicp.voxel_downsample(ref, ic.VOXEL_A)
    down_b = okicp.voxel_downsample(down_a, ic.VOXEL_B)
    want_counts = [len(ref), len(down_a), len(down_b)]
    a, b = K.PreSteps(), K.PreSteps()
    a.set_option("fused", fused), b.set_option("fused", fused)
    lohi = a.Ingest(*m.args)
    assert_regime(a, case)
    assert_decoded(a, m, lohi, okicp.ingest(*m.args))
    na = a.PreprocessIngested(rel, ext, ic.MAX_RANGE, min_range, deskew, dst=0)
    nb = b.Preprocess(xyz, st, rel, ext, ic.MAX_RANGE, min_range, deskew, dst=0)
    assert na == nb == len(ref) and 0 < na < m.n - m.n // 5
    np.testing.assert_array_equal(a.download(0), b.download(0))
    np.testing.assert_allclose(a.download(0), ref, rtol=0, atol=1e-11)
    if deskew and min_range == 0.0:  # the case bites: at least one (0, 0, 0) record survives, at the place the oracle moves it to
        zero = np.all(xyz == 0.0, axis=1)
        moved = okicp.se3_act(ext, okicp.preprocess(xyz[zero], st[zero], rel, ic.MAX_RANGE, min_range, True))
        assert len(moved) >= 1
        out = a.download(0)
        for p in moved:
            assert np.abs(out - p).max(axis=1).min() <= 1e-11
    ca, fa = a.Frame(None, None, rel, ext, ic.MAX_RANGE, min_range, deskew, ic.VOXEL_A, ic.VOXEL_B)
    cb, fb = b.Frame(xyz, st, rel, ext, ic.MAX_RANGE, min_range, deskew, ic.VOXEL_A, ic.VOXEL_B)
    assert ca == want_counts and cb == want_counts
    np.testing.assert_array_equal(fa, fb)
    np.testing.assert_allclose(fa, ref, rtol=0, atol=1e-11)
    assert_same_buffers(a, b)
    np.testing.assert_allclose(a.download(1), down_a, rtol=0, atol=1e-11)
    np.testing.assert_allclose(a.download(2), down_b, rtol=0, atol=1e-11)
    assert a.get_option("fused_frames") == fused and b.get_option("fused_frames") == fused
