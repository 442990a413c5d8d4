"""The host-side plan of an EvaluateUntil call (csrc/host/until_plan.h): the slot
table of an in-place cache rewrite against its contract, the stored-prefix
lookup and its start slots against a plain map, the first out-of-range prefix,
the identity-gather test and gather offsets against the naive loops, and the
start-node table image against its per-start-node definition
(tests/cpp/batch_plan_test.cc; no GPU calls)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "distributed_point_functions_amd", "lib")


def test_batch_plan(tmp_path):
    exe = tmp_path / "batch_plan_test"
    subprocess.run(["g++", "-O1", "-std=c++20", "-Wall", "-pthread",
                    f"-I{os.path.join(ROOT, 'include')}",
                    f"-I{os.path.join(ROOT, 'distributed_point_functions_amd', 'csrc', 'host')}",
                    os.path.join(ROOT, "tests", "cpp", "batch_plan_test.cc"), "-o", str(exe),
                    f"-L{LIB}", "-ldpf", "-ldpf_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, DPF_HOST_THREADS="8"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "chunks 8" in r.stdout
    assert "0 failures" in r.stdout
