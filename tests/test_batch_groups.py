"""The bookkeeping of batches that register several scans per launch (kinematic_icp_amd/csrc/kicp_batch_groups.hpp: which scans
make a lane's next group, completion from the front) as a stand-alone C++ program with the address and undefined-behaviour
sanitizers compiled in: tests/cpp/batch_groups_test.cpp.  No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grouping_of_a_batch_under_random_convergence_patterns(tmp_path):
    exe = str(tmp_path / "batch_groups_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "batch_groups_test.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "OK", run.stdout + run.stderr
