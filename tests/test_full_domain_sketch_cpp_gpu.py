"""Checked private histograms through the C++ API on the GPU:
tests/cpp/full_domain_sketch_api_test.cc, compiled against the public headers
only, compares EvaluateFullDomainSumSketch and
EvaluateFullDomainSumSketchToDevice with the per-key EvaluateUntil<T> vectors
summed and sketched on the host for IntModN<uint32_t, 2^32 - 5> and its
2-tuple (n = 9, 70 keys, both parties), reconstructs the histogram, recombines
the sketches, checks `accumulate` and the error codes."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "full_domain_sketch_api_test")


def test_cpp_full_domain_sum_sketch():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
