"""The 16-bit mirror's point format without a GPU (kicp_common.hpp::MirrorPoint: x and y as 16-bit integers, z as the float the pass
kernel subtracts the query from): tests/cpp/mirror_point_test.cpp holds the helpers to the format over all 65 536 z values, the empty
slot and the clamps; tests/cpp/mirror_host_test.cpp keeps HostMap::CheckInvariants() at 0 through random insertions and removals, with
re-used buckets reading empty behind their count.  Both are host-only programs of their own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, name):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    exe = str(tmp_path / name)
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert " 0 bad" in out.stdout
    return out.stdout


def test_the_z_word_is_the_float_of_the_quantised_z(tmp_path):
    _run(tmp_path, "mirror_point_test")


def test_host_map_keeps_its_invariants_through_insertions_and_removals(tmp_path):
    out = _run(tmp_path, "mirror_host_test")
    assert out.count("buckets re-used") == 3  # max_points_per_voxel 20, 21 and 40
