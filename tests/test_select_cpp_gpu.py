"""The C++ EvaluateSelect on the GPU: tests/cpp/select_api_test.cc answers two
XorWrapper<uint128> keys per party against a database of 2^13 three-word
records through the public headers only; every answer must equal
EvaluateUntil<T>'s bits folded on the host, the parties' answers must
recombine to the selected records, and two host errors must be reported."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "select_api_test")


def test_cpp_evaluate_select():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
