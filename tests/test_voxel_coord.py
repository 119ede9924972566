"""PointToVoxel with a constant guard, and the lane offsets taken from its fraction (kicp_pass_visit.hpp::voxel_coord, voxel_coord_offset),
without a GPU: tests/cpp/voxel_coord_test.cpp holds them to the formula they replaced, to the reference's floor(c / vs) and to the error
bound stated above start_lane, at voxel faces -+ 0 .. 4 ulps for k up to 2^20, either side of the guard, random coordinates and
|c / vs| just below 2^31.  A host-only program of its own, built with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_voxel_coord_equals_the_formula_it_replaced_and_the_offsets_keep_their_bound(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    exe = str(tmp_path / "voxel_coord_test")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "voxel_coord_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "voxel coord: 0 bad" in out.stdout
    m = re.search(r"(\d+) checked, (\d+) by division \((\d+) of them inside the new guard alone\), (\d+) offsets", out.stdout)
    checked, divided, only_now, bounded = map(int, m.groups())
    assert checked > 2_000_000 and divided > 100_000 and only_now > 1000 and bounded > 1_000_000
