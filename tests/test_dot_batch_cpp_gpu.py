"""The C++ EvaluateDotBatch on the GPU: tests/cpp/dot_batch_api_test.cc answers
three uint64_t keys per party against a database of 2^12 five-word records
through the public headers only; every answer must equal EvaluateUntil<T>
folded on the host, the parties' answers must recombine to beta * db[alpha],
and two host errors must be reported."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "dot_batch_api_test")


def test_cpp_evaluate_dot_batch():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
