"""The C++ MultipleIntervalContainmentGate on the GPU: tests/cpp/mic_gate_test.cc
restates the reference's Gen-and-Eval and error tests
(dcf/fss_gates/multiple_interval_containment_test.cc) through the reference's
public signatures only, so a C++ caller's drop-in path (Create, Gen, Eval with
messages built by hand) is covered as well as the Python mirror's."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "distributed_point_functions_amd", "lib", "mic_gate_test")


def test_cpp_mic_gate():
    assert os.path.exists(BIN), "build first: python -m distributed_point_functions_amd.build_native"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
