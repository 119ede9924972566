"""The order-preserving integer keys through which the ingest kernels fold the stamps' extrema
(kinematic_icp_amd/csrc/kicp_ordered_key.hpp: ordered_key / ordered_value) as a stand-alone C++ program with the address and
undefined-behaviour sanitizers compiled in: tests/cpp/ordered_key_test.cpp.  It checks the header's own two functions, where
tests/test_ingest.py re-enacts them in numpy.  No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ordered_keys_of_the_header_are_monotone_and_invertible(tmp_path):
    exe = str(tmp_path / "ordered_key_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "ordered_key_test.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "OK", run.stdout + run.stderr
