"""The batched private table lookup through the C++ API on the GPU:
tests/cpp/lookup_api_test.cc, compiled against the public headers only,
compares EvaluateLookupBatch with EvaluateUntil<T> folded into the rotated
table on the host for uint64_t and XorWrapper<uint64_t>, reconstructs
beta * T[(alpha + s) mod N] from the two parties' answers, and checks the error
codes."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "lookup_api_test")


def test_cpp_lookup_batch():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
