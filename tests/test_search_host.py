"""The whole-map relocalisation without a GPU: the host traversal (kicp_search_host.hpp) in a stand-alone program under ASan + UBSan
against the exhaustive top-M, the window helpers, and the inputs of tests/test_gpu_search.py pinned on the CPU alone.

Pins (tests/search_cases.py; the numpy restatement tests/search_ref.py over the doubles of K.search_yaws, map = the oracle's
Pointcloud()): per config and scan the exhaustive top-8 level-0 scores of the 64 x 64 x 180 window (737 280 nodes)
    cfg4, cell 0.05, scan 0 (250 keypoints): 54 53 52 52 51 51 42 41, the 9th 40; best node 0.022 m / 0.11 deg from the truth
    cfg4, cell 0.05, scan 1 (240):           46 45 42 41 41 40 40 40, the 9th 39
    cfg1, cell 0.25, scan 0 (854):           854 854 854 854 836 835 815 813 - four nodes tie at ALL keypoints: the score saturates on
                                             a dense map, which is why the truncated cost, not the score, picks the winner
    cfg1, cell 0.25, scan 1 (866):           860 855 846 841 825 820 815 811
all eight finalists of cfg1 within 0.474 m / 0.49 deg of the truth.  Refinement of the eight finalists on the oracle
(planar_ref.refine over okicp.associate, 100 iterations / 1e-4, cheapest by the truncated cost; tau = first_frame_tau() and twice
that) ends 0.003 .. 0.014 m / <= 0.05 deg from the truth on cfg4 and 0.031 m / 0.078 m, <= 0.06 deg on cfg1: inside one cell and one
yaw step, the condition the GPU test asserts."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
from oracle import okicp
import planar_ref as pr
import search_cases as sc
import search_ref as sr


def test_search_traversal_stand_alone_under_sanitizers(tmp_path):
    """kicp_search_host.hpp in a program of its own (tests/cpp/search_host_test.cpp), ASan + UBSan, as a subprocess"""
    exe = str(tmp_path / "search_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "search_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.strip().startswith("ok "), out.stdout[-2000:]
    assert int(out.stdout.split()[1]) > 100000


def test_search_yaws_and_window_arguments():
    w = K.SearchWindow(1.0, 2.0, 0.5, 3, 4, -0.3, 0.01, 7)
    assert w.nodes == 84
    cs = K.search_yaws(w)
    want = np.array([[np.cos(-0.3 + float(j) * 0.01), np.sin(-0.3 + float(j) * 0.01)] for j in range(7)])
    np.testing.assert_allclose(cs, want, rtol=0, atol=2.3e-16)  # (two libms: an ulp; the tests feed the restatement THESE doubles)
    for bad in (K.SearchWindow(0, 0, 0, 0, 4, 0, 0.1, 1), K.SearchWindow(0, 0, 0, 4, 4, 0, 0.1, 0), K.SearchWindow(0, 0, 0, 4, (1 << 20) + 1, 0, 0.1, 1),
                K.SearchWindow(np.nan, 0, 0, 4, 4, 0, 0.1, 1)):
        with pytest.raises(K.KicpError) as e:
            K.search_yaws(bad)
        assert e.value.code == K.KICP_ERR_ARG


def test_restatement_bounds_and_packing():
    """the restatement's own invariants: level h at a cell covers level 0 at every cell of the block, and the word layout"""
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1.0, 1.0, (40, 3)) * np.array([3.0, 2.0, 0.2])
    mn, dims, levels = sr.pyramid(pts, 0.1, 1, 4)
    assert not levels[0][:, :, 0].any() and not levels[0][:, 0, :].any() and not levels[0][:, :, -1].any()  # the margins stay empty
    for h in range(1, 5):
        for _ in range(200):
            x, y, z = (int(rng.integers(0, d)) for d in dims)
            block = levels[0][z, y:y + (1 << h), x:x + (1 << h)]
            assert levels[h][z, y, x] == block.any()
    words = sr.pack(levels[0])
    assert words.dtype == np.uint32 and words.shape == (dims[2], dims[1], (dims[0] + 31) // 32)
    z, y, x = np.argwhere(levels[0])[7]
    assert (int(words[z, y, x >> 5]) >> (x & 31)) & 1
    assert int(sum(bin(int(v)).count("1") for v in words.reshape(-1))) == int(levels[0].sum())


@pytest.mark.parametrize("name", ["cfg4", "cfg1"])
def test_pinned_inputs_on_the_cpu_alone(name):
    cfg, omap, items = sc.case(name)
    cell = sc.CELL[name]
    mn, dims, levels = sr.pyramid(omap.Pointcloud(), cell, sc.DILATE, sc.LEVELS)
    for scan, (keypoints, truth, window) in enumerate(items):
        n = len(keypoints)
        assert n == sc.KEYPOINTS[(name, scan)]
        cells = sr.frame_cells(keypoints, K.search_yaws(window), window, mn, cell)
        scores = sr.score_window(levels[0], cells, window)
        nodes, hits = sr.top_m(scores, sc.TOP_M + 1)
        want, ninth = sc.PINNED_HITS[(name, scan)]
        assert hits[:sc.TOP_M].tolist() == want and (ninth is None or hits[sc.TOP_M] == ninth)
        assert np.array_equal(sr.score_nodes(levels[0], cells, window, nodes), hits)  # the two ways of scoring agree
        # every bound of the top level holds for the best nodes' blocks
        top = levels[sc.LEVELS]
        blocks = (nodes // window.nx // window.ny * window.ny + (nodes // window.nx % window.ny) // 16 * 16) * window.nx + (nodes % window.nx) // 16 * 16
        assert (sr.score_nodes(top, cells, window, blocks, h=sc.LEVELS) >= hits).all()
        finalists = [sr.node_pose(window, cell, nd) for nd in nodes[:sc.TOP_M]]
        offsets = [sc.offset(truth, p) for p in finalists]
        if (name, scan) == ("cfg4", 0):
            assert round(offsets[0][0], 3) == 0.022 and round(np.degrees(offsets[0][1]), 2) == 0.11
        if name == "cfg1":
            assert max(o[0] for o in offsets) < 0.4745 and max(np.degrees(o[1]) for o in offsets) < 0.495
        for tau in (cfg.first_frame_tau(), 2.0 * cfg.first_frame_tau()):
            best = None
            for start in finalists:
                pose, iterations, status = pr.refine(lambda p: okicp.associate(omap, keypoints, p, tau)[:2], keypoints, start, 100, 1e-4)
                assert status == pr.CONVERGED
                after = okicp.icp_pass(omap, keypoints, pose, tau)[0]
                c = (after[5] + (float(n) - after[6]) * (tau * tau)) / float(n)
                if best is None or c < best[0]:
                    best = (c, pose)
            d, yaw = sc.offset(truth, best[1])
            print("%s scan %d tau %.3f: %.4f m, %.4f deg from the truth" % (name, scan, tau, d, np.degrees(yaw)))
            assert d < cell and yaw < sc.YAW_STEP  # within one cell and one yaw step: the condition the GPU test asserts
