"""The owning buffer types of csrc/kicp_internal.hpp (DevBuf, PinnedBuf, HostStage): what a FAILED growth leaves behind, moves,
swap and release (tests/cpp/buffers_test.cpp).  The failure path needs a machine without a GPU - every allocation fails there -, so
the program is built and run only where no device is visible: a stand-alone program, its host code under ASan + UBSan, run directly."""
import os
import subprocess

import pytest

from conftest import ROOT
import kinematic_icp_amd as K


def test_failed_growth_leaves_the_buffers_empty(tmp_path):
    if K.device_count() > 0:
        pytest.skip("a GPU is present: allocations succeed, the failure path cannot be reached")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(ROOT, "kinematic_icp_amd", "csrc")
    exe = str(tmp_path / "buffers_test")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Wall", "-Wextra",
                           "-Wno-unused-parameter", "-Wno-unused-value", "-Wno-unused-function", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "buffers_test.cpp"), os.path.join(csrc, "kicp_core.hip"),
                           "-o", exe, "-ldl"])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stderr == "", p.stderr  # (a sanitizer report)
    assert p.stdout.startswith("ok "), p.stdout
    assert int(p.stdout.split()[1]) > 60
