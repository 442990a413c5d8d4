"""The fused full-domain sum over a key batch through the C++ API on the GPU:
tests/cpp/full_domain_sum_api_test.cc, compiled against the public headers
only, compares EvaluateFullDomainSum and EvaluateFullDomainSumToDevice with the
per-key EvaluateUntil<T> vectors summed on the host for uint64_t and
XorWrapper<uint64_t> (n = 9, 70 keys, both parties), reconstructs the
histogram, checks `accumulate` and the error codes."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "full_domain_sum_api_test")


def test_cpp_full_domain_sum():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
