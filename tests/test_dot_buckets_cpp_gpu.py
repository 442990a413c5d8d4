"""Multi-query PIR over a bucketed database through the C++ API on the GPU:
tests/cpp/dot_buckets_api_test.cc, compiled against the public headers only,
compares EvaluateDotBuckets with EvaluateDot<T> of every key on its bucket's
slice for uint64_t and XorWrapper<uint64_t>, reconstructs
beta * db[b(k)][alpha] from the two parties' answers, and checks the error
codes."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "dot_buckets_api_test")


def test_cpp_dot_buckets():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
