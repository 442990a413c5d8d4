#!/usr/bin/env python3
"""When do the waves of a full-domain expand launch leave the kernel?

Runs bench.py's full-domain uint64 workload one launch at a time with the clock
probe on and prints, per configuration, the medians over the launches of
  * the launch's span (first workgroup begin to last wave exit),
  * first wave exit to last wave exit, as a share of the span: the drain
    during which the LDS pipes run on fewer and fewer waves,
  * earliest to latest of the workgroups' last exits, as a share of the span:
    the skew between compute units.
Set the DPF_OCTET_* hooks in the environment to compare schedules.

Usage: python tools/exit_spread.py [--log-domain 30] [--rehearse-world 8] [--launches 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-domain", type=int, default=30)
    ap.add_argument("--rehearse-world", type=int, default=1)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import hip_abi as H
    from distributed_point_functions_amd import proto as pb
    from distributed_point_functions_amd import sharding as S

    H.load(require_gpu=True)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    params = pb.DpfParameters()
    params.log_domain_size = a.log_domain
    params.value_type.CopyFrom(D.integer_type(64))
    dpf = D.DistributedPointFunction.create(params)
    key, _ = dpf.generate_keys_incremental(
        0x2545F4914F6CDD1D % (1 << a.log_domain), [D.to_value(D.integer_type(64), 0xDEADBEEF)],
        seeds=(0x243F6A8885A308D3, 0x13198A2E03707344))   # bench.py's key
    ctx0 = dpf.create_evaluation_context(key)
    shards = a.rehearse_world
    outputs = 1 << S.strong_scaling_log_outputs(a.log_domain, shards)
    out = torch.empty(outputs * 8, dtype=torch.uint8, device=dev)

    def launch():
        ctx = pb.EvaluationContext()
        ctx.CopyFrom(ctx0)
        assert dpf.evaluate_shard_to_device(0, 0, shards, ctx, out, stream=stream) == outputs

    for _ in range(a.warmup):
        launch()
    torch.cuda.synchronize(dev)
    H.clock_probe(True)
    rows = []
    for _ in range(a.launches):
        launch()
        e = H.clock_probe_exits()      # waits for the device
        c = H.clock_probe_read()       # zeroes the stamps for the next launch
        span = e["last_exit_ms"]
        rows.append({
            "span_ms": span,
            "first_exit_ms": e["first_exit_ms"],
            "drain_share": (span - e["first_exit_ms"]) / span if span else 0.0,
            "workgroup_skew_share": (e["workgroup_last_exit_max_ms"]
                                     - e["workgroup_last_exit_min_ms"]) / span if span else 0.0,
            "workgroup_last_exit_mean_share": e["workgroup_last_exit_mean_ms"] / span if span else 0.0,
            "wave0_mean_ms": c["mean_workgroup_ms"],
            "clock_ghz": c["clock_ghz"],
            "workgroups": e["workgroups"],
        })
    H.clock_probe(False)
    med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    med.update(log_domain=a.log_domain, rehearse_world=shards, launches=a.launches,
               kernel=H.last_expand_kernel()[0],
               hooks={k: v for k, v in os.environ.items() if k.startswith("DPF_OCTET_")})
    print(json.dumps(med))


if __name__ == "__main__":
    main()
