"""The premises of tests/egress_cases.py, proved on the CPU from the oracle and the restated piece rules alone, so that the regime
each case of tests/test_gpu_egress_regimes.py claims - a piece that ends on a boundary, a tail of a few words, a bucket deeper
than an LDS round, a slot used twice - is a property of its input.  The rules are restated there, not imported: the constants they
rest on are read here out of the sources as text, so that a changed constant fails here instead of silently uncovering a regime."""
import os
import re

import numpy as np
import pytest

import egress_cases as ec
import prestep_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kinematic_icp_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def constant(text, name):
    m = re.search(r"constexpr\s+(?:static\s+)?(?:u?int(?:32_t)?|size_t)\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, name
    return int(m.group(1))


def test_the_restated_rules_rest_on_the_sources_constants():
    assert constant(source("kicp_pre_shared.hpp"), "kPushPieces") == ec.PUSH_PIECES == 8
    assert constant(source("kicp_map_pc.hpp"), "kPcRoundRecords") == ec.MAP_ROUND == 2048
    assert constant(source("kicp_internal.hpp"), "kRecSlots") == ec.MAP_SLOTS == 4
    egress, kernels, mapsrc = source("kicp_pre_egress.hip"), source("kicp_pre_egress.hpp"), source("kicp_map_cloud.hip")
    # the frame's piece size, the default grid and what one workgroup stores per sweep
    assert "((n_in * job.rec_bytes + kPushPieces - 1) / kPushPieces + 4095) / 4096 * 4096" in egress
    assert 'env_int("KICP_PRE_PUSH_WGS", 16)' in egress and "if (len < job.piece_bytes) break;" in egress
    assert kernels.count("static_cast<size_t>(gridDim.x) * 4096u") == 2 and ec.PUSH_SWEEP == 16 * 4096
    assert "std::min<size_t>((words + 255) / 256, 1024)" in egress and ec.NARROW_GRID_WORDS == 1024 * 256
    # the map's piece rule
    assert "std::min<size_t>(65536, std::max<size_t>(1024, ((want + kSlots - 1) / kSlots + 1023) / 1024 * 1024))" in mapsrc
    assert (ec.MAP_PIECE_MIN, ec.MAP_PIECE_MAX) == (1024, 65536)
    assert "calls of 4096 points or more" in open(os.path.join(ROOT, "include", "kicp.h")).read() and ec.BULK == 4096


def test_the_frames_piece_rule():
    assert [ec.frame_piece_bytes(n, r) for n, r in ((1, 24), (1365, 24), (1366, 24), (4096, 24), (2730, 12), (2731, 12), (44000, 12), (40000, 24))] == \
        [4096, 4096, 8192, 12288, 4096, 8192, 69632, 122880]
    assert ec.frame_pieces(0, 300, 24) == [0] * 8 and ec.frame_pieces_followed(0, 300, 24) == 1
    assert ec.frame_pieces(171, 1365, 24) == [4096, 8, 0, 0, 0, 0, 0, 0] and ec.frame_pieces_followed(171, 1365, 24) == 2
    assert ec.frame_pieces(512, 1365, 24) == [4096, 4096, 4096, 0, 0, 0, 0, 0] and ec.frame_pieces_followed(512, 1365, 24) == 4
    assert ec.frame_pieces(4096, 4096, 24) == [12288] * 8 and ec.frame_pieces_followed(4096, 4096, 24) == 8
    for n_in in (1, 300, 1365, 4096, 44000):
        for rec in (12, 24):  # eight pieces always hold the whole input
            assert sum(ec.frame_pieces(n_in, n_in, rec)) == n_in * rec and ec.frame_piece_bytes(n_in, rec) % 4096 == 0


@pytest.mark.parametrize("case", ec.PUSH_CASES, ids=repr)
def test_pieces_of_a_push_case(case):
    """the written-out pieces are the rule's, the worker's view is the first short piece; the regime the case is named after"""
    piece = ec.frame_piece_bytes(case.n_in, case.rec_bytes)
    assert ec.frame_pieces(case.n0, case.n_in, case.rec_bytes) == case.pieces and len(case.pieces) == 8
    assert sum(case.pieces) == case.n0 * case.rec_bytes
    short = [i for i, length in enumerate(case.pieces) if length < piece]
    assert case.followed == (short[0] + 1 if short else 8) == ec.frame_pieces_followed(case.n0, case.n_in, case.rec_bytes)


def test_the_push_table_is_the_issues():
    table = [(c.rec_bytes, c.n_in, c.n0) for c in ec.PUSH_CASES]
    assert table == [(24, 1365, 170), (24, 1365, 171), (24, 1365, 512), (24, 1365, 1365), (24, 4096, 4096), (24, 4096, 4095), (24, 300, 0),
                     (12, 2730, 1), (12, 2730, 2), (12, 2730, 3), (12, 2730, 4), (12, 2730, 341), (12, 2730, 342), (12, 2730, 1024),
                     (12, 8192, 8192), (12, 8192, 0), (12, 44000, 22909)]
    by = {t: c for t, c in zip(table, ec.PUSH_CASES)}
    assert by[(24, 1365, 170)].pieces == [4080, 0, 0, 0, 0, 0, 0, 0]
    assert by[(24, 1365, 171)].pieces == [4096, 8, 0, 0, 0, 0, 0, 0]
    assert by[(24, 1365, 512)].pieces == [4096, 4096, 4096, 0, 0, 0, 0, 0] == by[(12, 2730, 1024)].pieces
    assert by[(24, 1365, 1365)].pieces == [4096] * 7 + [4088]
    assert by[(24, 4096, 4096)].pieces == [12288] * 8 == by[(12, 8192, 8192)].pieces
    assert by[(24, 4096, 4095)].pieces == [12288] * 7 + [12264]
    assert [by[(12, 2730, n)].pieces[0] for n in (1, 2, 3, 4, 341)] == [12, 24, 36, 48, 4092]  # 4 092: a three-word tail
    assert by[(12, 2730, 342)].pieces[:2] == [4096, 8]
    assert ec.EXACT_BOUNDARY == [by[(24, 1365, 512)], by[(12, 2730, 1024)]] and ec.ALL_FULL == [by[(24, 4096, 4096)], by[(12, 8192, 8192)]]
    # the last row: a piece beyond one sweep of sixteen workgroups, the last one longer than the sweep, ending off a unit
    big = by[(12, 44000, 22909)]
    assert big.n_in > 43690 and ec.frame_piece_bytes(44000, 12) == ec.BIG_PIECE == 69632 > ec.PUSH_SWEEP
    last = big.pieces[big.followed - 1]
    assert ec.PUSH_SWEEP < last < ec.BIG_PIECE and last % 16 == 12 and last - last % 16 > ec.PUSH_SWEEP
    # stale flags: the 40 000-point frame's pieces are longer than every case's piece size, and it fills several of them
    stale = ec.frame_pieces(ec.STALE_MAKER.n0, ec.STALE_MAKER.n_in, 24)
    assert ec.STALE_MAKER.n_in == 40000 and stale[:5] == [122880] * 5 and 0 < stale[5] < 122880
    assert all(ec.frame_piece_bytes(c.n_in, c.rec_bytes) < 122880 for c in ec.PUSH_CASES)
    assert all(ec.frame_piece_bytes(c.n_in, r) < 122880 for c in ec.PUSH_CASES[:16] for r in (12, 24))  # (44 000 points as doubles: 135 168)
    # one handle over time; the DMA route's two modes (kicp_pre_egress.hip transfer_piece_bytes: pieces from 1 MiB on)
    assert [c.n_in for c in ec.SEQUENCE] == [300, 44000, 1365, 4096, 300]
    sizes = [ec.frame_piece_bytes(c.n_in, 24 if k % 2 == 0 else 12) for k, c in enumerate(ec.SEQUENCE)]
    assert sizes[2] < sizes[1] > sizes[3] and sizes[4] < sizes[3]  # the piece size shrinks between launches
    assert ec.DMA_PIECES.n_in * 24 >= 1 << 20 > ec.DMA_ONE_EVENT.n_in * 24
    # the landing area (landing_reserve: half as much again and 1 MiB) holds every frame of the sequence behind the first, not the 50 000
    assert "p->egress.host.reserve(bytes + bytes / 2 + (1u << 20)" in source("kicp_pre_egress.hip")
    room = ec.LANDING_FIRST.n_in * 24 * 3 // 2 + (1 << 20)
    assert max(c.n_in for c in ec.SEQUENCE) * 24 <= room < ec.LANDING_GROWS.n_in * 24


@pytest.mark.parametrize("case", ec.PUSH_CASES + [ec.DMA_PIECES, ec.LANDING_GROWS, ec.KP_ONE_HIT, ec.KP_ONE_MISS], ids=repr)
def test_counts_of_a_frame_case(case):
    """as tests/test_prestep_cases.py: the oracle chain's counts are the pinned ones and a plain numpy count's"""
    pts = case.build()
    b0, b1, b2 = pc.oracle_chain(case)
    counts = pc.numpy_counts(pts, case.max_range, case.min_range, case.voxel_a, case.voxel_b)
    assert pts.shape == (case.n_in, 3) and [len(b0), len(b1), len(b2)] == case.counts == counts
    assert case.counts[:2] == [case.n0, case.n1] and (case.pinned_n2 is None or case.counts[2] == case.pinned_n2)
    r = np.sqrt((pts * pts).sum(axis=1))
    assert np.all((np.abs(r - case.max_range) > 1.0) & (np.abs(r - case.min_range) > 1.0))
    assert np.array_equal(b0, pts[r < case.max_range])
    for v in (case.voxel_a, case.voxel_b):
        frac = b0 / v - np.floor(b0 / v)
        assert np.all((frac > 0.1) & (frac < 0.9))
    if case.n0 > case.n1 > 0:
        assert len(np.unique(b0, axis=0)) == case.n0
    narrowed = b0.astype(np.float32).astype(np.float64)
    assert case.n0 == 0 or np.any(narrowed != b0)  # (narrowing changes the numbers: a frame of doubles is not its records)


def test_the_keypoint_cases():
    assert [c.n2 for c in ec.KEYPOINT_CASES[:3]] == [0, 1, 1] and ec.KP_NONE.n0 == 0 and ec.KP_NONE.hit
    assert ec.KP_ONE_HIT.hit and not ec.KP_ONE_MISS.hit and ec.KP_ONE_HIT.build() is not ec.KP_ONE_MISS.build()
    assert np.array_equal(ec.KP_ONE_HIT.build(), ec.KP_ONE_MISS.build())  # the same cloud, guessed 20 / 257: 64 buckets / 1 024
    assert (pc.buckets(20), pc.buckets(257), ec.KP_ONE_MISS.spec_buckets()) == (64, 1024, 1024)
    assert ec.KP_HIT.hit and not ec.KP_MISS.hit and (ec.KP_HIT.n0, ec.KP_MISS.n0, ec.KP_MISS.guess) == (4096, 4096, 4097)
    assert ec.KP_HIT.n2 > 256  # an ordinary frame's keypoints
    # k_narrow_f32: 1 024 workgroups of 256 lanes narrow 262 144 words a turn
    assert 3 * ec.NARROW_SIZES[1] < ec.NARROW_GRID_WORDS < 3 * ec.NARROW_SIZES[2] and ec.NARROW_SIZES[2] - ec.NARROW_SIZES[1] == 1
    assert ec.NARROW_GROW * 3 > ec.NARROW_GRID_WORDS > ec.NARROW_REUSE * 3
    p = ec.narrow_points(1000)
    assert np.any(p.astype(np.float32).astype(np.float64) != p) and np.abs(p).max() < 1e6


def test_the_maps_piece_rule():
    assert [ec.map_piece_records(w) for w in (1, 5, 4096, 4097, 8192, 8193, 262144, 262145, 1 << 20)] == \
        [1024, 1024, 1024, 2048, 2048, 3072, 65536, 65536, 65536]
    assert [ec.map_pieces(w) for w in (0, 1, 5, 1024, 1025, 4096, 4097, 262144, 262145, 1 << 20)] == [0, 1, 1, 1, 2, 4, 3, 4, 5, 16]
    assert [ec.map_pieces(w) for w in ec.PIECE_EDGE_CAPS] == [4, 3, 4, 5]  # 262 145: slot 0 used a second time
    for w in (1, 4096, 4097, 262145, 999999):
        assert ec.map_piece_records(w) % 4 == 0 and ec.map_pieces(w) * ec.map_piece_records(w) >= w


def voxel_of(cloud, voxel):
    return np.floor(cloud / voxel).astype(np.int64)


def test_the_deep_bucket_scene():
    scene = ec.deep_bucket()
    cloud = ec.oracle_map_cloud(scene)
    assert all(len(c[1]) >= ec.BULK for c in scene.calls) and scene.cap == ec.DEEP_CAP > ec.MAP_ROUND
    deep = (voxel_of(cloud, scene.voxel) == np.array(ec.DEEP_VOXEL)).all(axis=1)
    assert deep.sum() == ec.DEEP_POINTS == 4500 > 2 * ec.MAP_ROUND and len(cloud) == 4500 + 600  # nothing was refused, nothing pruned
    assert max(ec.DEEP_CUTS) < ec.DEEP_POINTS and ec.DEEP_CUTS[:3] == (ec.MAP_ROUND - 1, ec.MAP_ROUND, ec.MAP_ROUND + 1)
    _, per_voxel = np.unique(voxel_of(cloud[~deep], scene.voxel), axis=0, return_counts=True)
    assert per_voxel.max() == 1


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_a_few_points_scene(k):
    scene = ec.few_points(k)
    cloud = ec.oracle_map_cloud(scene)
    assert all(len(c[1]) >= ec.BULK for c in scene.calls) and scene.cap == 1
    assert len(cloud) == k and len(np.unique(voxel_of(cloud, scene.voxel), axis=0)) == k
    assert 3 * k < 16  # fewer than four 16-byte units; one record: fewer words than one unit
    assert np.all(np.sqrt((cloud * cloud).sum(axis=1)) < scene.max_distance - 1.0)


def test_the_sparse_scene():
    scene = ec.sparse()
    cloud = ec.oracle_map_cloud(scene)
    assert all(len(c[1]) >= ec.BULK for c in scene.calls)
    assert 150 < len(cloud) < 700  # of the 40 000 (a table sized for them: at least 80 000 slots, 300 blocks and more)
    assert len(np.unique(voxel_of(cloud, scene.voxel), axis=0)) > 100


def test_the_piece_edges_scene():
    scene = ec.piece_edges()
    cloud = ec.oracle_map_cloud(scene)
    assert all(len(c[1]) >= ec.BULK for c in scene.calls)
    assert len(cloud) >= 262145 == max(scene.caps) and ec.map_pieces(len(cloud)) == 5
    assert [s.name for s in ec.map_scenes()] == ["deep_bucket"] + ["few_points_%d" % k for k in range(1, 6)] + ["sparse", "piece_edges"]
