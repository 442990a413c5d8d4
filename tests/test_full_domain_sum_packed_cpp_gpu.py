"""The packed full-domain sum through the C++ API on the GPU:
tests/cpp/full_domain_sum_packed_api_test.cc, compiled against the public
headers only, compares EvaluateFullDomainSumPacked<T> and its ToDevice form
with the per-key EvaluateUntil<T> vectors summed on the host for uint32_t,
uint8_t (n = 9) and XorWrapper<uint128> (n = 7), 70 keys, both parties,
reconstructs the histogram, and checks the status codes of a wrong T, an
unsupported type or shape and a foreign batch."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib",
                   "full_domain_sum_packed_api_test")


def test_cpp_full_domain_sum_packed():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
