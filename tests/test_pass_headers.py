"""Every header the pass kernels are cut into compiles ON ITS OWN, without a GPU: a one-line file that includes nothing but the header goes
through hipcc -fsyntax-only twice, as host code and as gfx950 device code.  A header that leans on something its includer happened to
include first (a struct of kicp_pass_params.hpp, kNoIndex32 of kicp_nn_exact.hpp, <cfloat>) fails here and nowhere else: every
translation unit of the library includes several of them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kinematic_icp_amd", "csrc")
HEADERS = ["kicp_pass_params.hpp", "kicp_pass_fixed.hpp", "kicp_nn_exact.hpp", "kicp_pass_finish.hpp", "kicp_pass_visit.hpp", "kicp_kernels.hpp",
           "kicp_map_kernels.hpp"]
SIDES = {"host": ["--cuda-host-only"], "device": ["--cuda-device-only", "--offload-arch=gfx950"]}


@pytest.mark.parametrize("side", sorted(SIDES))
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(tmp_path, header, side):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    assert os.path.exists(os.path.join(CSRC, header))
    one_line = tmp_path / "only_this_header.hip"
    one_line.write_text('#include "%s"\n' % header)
    out = subprocess.run([hipcc, "-x", "hip", "-std=c++17", "-fsyntax-only", "-I", CSRC] + SIDES[side] + [str(one_line)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
