"""The host-side plan of the shard, dot, select and split calls
(csrc/host/shard_plan.h): the slab plan against the two loops it replaced over
every tree depth, value type, key count and hook value, the shard split
against its definition with its messages and the 2^62 boundary, and the
subtree paths (tests/cpp/shard_plan_test.cc; no GPU calls)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_plan(tmp_path):
    exe = tmp_path / "shard_plan_test"
    subprocess.run(["g++", "-O1", "-std=c++20", "-Wall", "-Wextra",
                    f"-I{os.path.join(ROOT, 'include')}",
                    f"-I{os.path.join(ROOT, 'distributed_point_functions_amd', 'csrc', 'host')}",
                    os.path.join(ROOT, "tests", "cpp", "shard_plan_test.cc"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 40 depths x 44 hook values x (2 dot types + 64 key counts)
    assert "slab cases 116160" in r.stdout
    assert "0 failures" in r.stdout
