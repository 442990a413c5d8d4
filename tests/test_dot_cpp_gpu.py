"""The C++ template EvaluateDot<T> on the GPU: tests/cpp/dot_api_test.cc folds
uint64_t and XorWrapper<uint128> keys of a 2^12 domain into a database of
4-word records through the public headers only; both parties must reconstruct
record alpha, and uint32_t must be UNIMPLEMENTED."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "dot_api_test")


def test_cpp_evaluate_dot():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
