"""The C++ batched key generators on the GPU: tests/cpp/keygen_api_test.cc
generates DPF, DCF and MIC key batches on the device through the public headers
only, downloads them, and compares every row with the single-key ...WithSeeds
call; a downloaded batch survives SerializeKeyBatch then ParseKeyBatch, and two
host errors must be reported."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "keygen_api_test")


def test_cpp_batched_key_generation():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
