"""Full-domain DCF evaluation through the C++ API on the GPU:
tests/cpp/dcf_expand_api_test.cc, compiled against the public headers only,
compares EvaluateFullDomain<uint64_t> with a loop of Evaluate<uint64_t>,
reconstructs a range query from EvaluateRangeDot's two answers, and expects
UNIMPLEMENTED for an IntModN DCF."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "dcf_expand_api_test")


def test_cpp_full_domain_dcf():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
