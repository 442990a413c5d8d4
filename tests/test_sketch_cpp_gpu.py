"""The C++ EvaluateUntilBatchSketchToDevice on the GPU: tests/cpp/sketch_api_test.cc
sketches 70 Tuple<IntModN32, IntModN32> key pairs over a 3-level hierarchy
through the public headers only; every sketch must equal EvaluateUntil<T>
folded with the weights on the host, the sums the host sum, the parties'
sketches must recombine to w[j][i*] * beta, and two host errors must be
reported."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "sketch_api_test")


def test_cpp_evaluate_until_batch_sketch():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
