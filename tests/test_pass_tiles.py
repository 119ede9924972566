"""What the pass kernel's tiles rest on that a CPU can check (kinematic_icp_amd/csrc/kicp_pass_tiles.hpp: the row words of a
workgroup's limb sums against 128-bit arithmetic, the automatic tile count, the option's clamp) as a stand-alone C++ program with
the address and undefined-behaviour sanitizers compiled in: tests/cpp/pass_tiles_test.cpp.  No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_words_and_the_automatic_tile_count(tmp_path):
    exe = str(tmp_path / "pass_tiles_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pass_tiles_test.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "OK", run.stdout + run.stderr
