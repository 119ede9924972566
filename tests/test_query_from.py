"""The query's offset from a neighbour voxel's corner (kicp_pass_visit.hpp::axis_from, query_from), without a GPU:
tests/cpp/query_from_test.cpp holds the three-instruction form to the float of the form it replaced, l - d 65536 from the integer
component, for every shift and axis over all 2^16 integer offsets, fractions beside them and random offsets.  A host-only program of
its own, built with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_axis_from_gives_the_float_of_the_form_it_replaced(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    exe = str(tmp_path / "query_from_test")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "query_from_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"query from: (\d+) bad of (\d+) checked", out.stdout)
    bad, checked = map(int, m.groups())
    assert bad == 0 and checked > 81 * 65536 * 10
