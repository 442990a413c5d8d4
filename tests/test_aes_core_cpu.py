"""The entry points of csrc/kernels/aes_core.h on the host (HostLookup + ArrayRK):
encrypt against FIPS-197 Appendix C.1, mmo_hash against tests/golden/aes_kat.json,
and the interleaved forms (encrypt2, encryptN<1..4>, encryptAB<2,2>, mmo_hash2,
mmo_hashN, mmo_hashAB) block by block against the single-block ones
(tests/cpp/aes_core_test.cc; g++ only, no GPU library)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_aes_core(tmp_path):
    exe = tmp_path / "aes_core_test"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall",
                    f"-I{os.path.join(ROOT, 'distributed_point_functions_amd', 'csrc', 'kernels')}",
                    os.path.join(ROOT, "tests", "cpp", "aes_core_test.cc"), "-o", str(exe)],
                   check=True)
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "aes_kat.json")))
    args = []
    for case in kat["cases"]:
        for x, y in zip(case["in"], case["out"]):
            args += [f"{int(v, 16):032x}" for v in (case["key"], x, y)]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    n = sum(len(case["in"]) for case in kat["cases"])
    assert n >= 4
    assert f"aes_core: {n} known answers, 64 blocks, 0 failures" in r.stdout
