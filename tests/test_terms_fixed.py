"""The pass kernels' five terms through terms_to_fixed (kicp_pass_fixed.hpp) against five to_fixed calls, without a GPU:
tests/cpp/terms_fixed_test.cpp compares all twenty limbs and the range flag at zeros, ties, both sides of the short path's limit 2^22,
the range limit 2^43, NaN and infinities in every position, 10^5 random values per binade from 2^-45 to 2^44 and mixtures with one
large term.  A host-only program of its own, built with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_terms_to_fixed_equals_five_to_fixed_calls_on_either_path(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    exe = str(tmp_path / "terms_fixed_test")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "terms_fixed_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"terms fixed: (\d+) bad of (\d+) sets checked, (\d+) on the short path, (\d+) on the general one, (\d+) with the range flag", out.stdout)
    bad, checked, short, general, flagged = map(int, m.groups())
    assert bad == 0
    # 89 binades of 20 000 sets: 67 of them lie below 2^22
    assert checked > 1_800_000 and short > 1_300_000 and general > 400_000 and flagged > 20_000
