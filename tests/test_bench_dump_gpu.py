"""A plain `bench.py` run on the GPU: the line carries the headline figure and
none of the --full legs, and `--dump-outputs` writes what the last timed step
left in HBM.

At log-domain 22 the 32 MiB of uint64 outputs are over bench.DUMP_WHOLE_BYTES,
so the dump is the seeded sample; every sampled output is compared with the
oracle's EvaluateUntil(0, {}) of the same key (bench.benchmark_key: fixed
alpha, beta and root seeds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = 22


def test_plain_run_dumps_the_last_step_outputs(tmp_path):
    import oracle as O
    import bench
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import proto as pb

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--log-domain", str(LOG), "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "u64" and d["unit"] == "leaves/s"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx((1 << LOG) / (d["ms_per_step"] * 1e-3), rel=1e-6)
    assert "cpu_baseline" not in d and "api_level" not in d     # --full only

    assert sorted(os.listdir(tmp_path)) == ["outputs.npy", "outputs_index.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20
    idx = np.load(tmp_path / "outputs_index.npy")
    got = np.load(tmp_path / "outputs.npy")
    assert idx.dtype == got.dtype == np.float64 and got.shape == (len(idx), 2)
    assert idx[0] == 0 and idx[-1] == (1 << LOG) - 1 and np.all(np.diff(idx) > 0)

    params = pb.DpfParameters()
    params.log_domain_size = LOG
    params.value_type.CopyFrom(D.integer_type(64))
    dpf = D.DistributedPointFunction.create(params)
    _, key = bench.benchmark_key(dpf, LOG, D.to_value(D.integer_type(64), 0xDEADBEEF))
    P = O.OracleParams([(LOG, ("int", 64), 0)])
    want = O.evaluate_until(P, 0, [], O.create_context(P, bench._oracle_key(key)))
    want = np.ascontiguousarray(want).view(np.uint32).reshape(1 << LOG, 2)[idx.astype(np.int64)]
    assert np.array_equal(got, want.astype(np.float64))
