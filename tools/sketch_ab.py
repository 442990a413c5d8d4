#!/usr/bin/env python3
"""Same-box, same-session timing of a heavy-hitters pass with per-client
sketches: HIP events around each whole pass (both servers, all
61 levels of the 128-bit hierarchy, top_k candidates), a warm-up, then
`--reps` rounds in which the variants alternate.  Timing only: parity is the
tests' job, though every sketch pass must flag no client.

  python tools/sketch_ab.py [--log-clients 18] [--reps 3] [-o profiles/r25/sketch_ab.txt]

  (a) sum     EvaluateUntilBatchSumToDevice at every level (no sketches)
  (b) fused   EvaluateUntilBatchSketchToDevice, J = 2: sums and sketches from
              hh_keys_sketch_kernel at every steady-state level
  (c) stream  the same call with DPF_BATCH_SKETCH_FUSED=0: per-key rows,
              dpf_hip_sketch_rows and dpf_hip_sum_rows
One JSON line per variant: median, min and max seconds per pass and the ratio
of the median to (a)'s.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-clients", type=int, default=18)
    ap.add_argument("--top-k", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("-o", "--output", help="also append the lines to this file")
    a = ap.parse_args()

    import numpy as np
    import torch
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import heavy_hitters as HH
    from distributed_point_functions_amd import hip_abi as H
    H.load(require_gpu=True)
    dev = torch.device("cuda")
    s = torch.cuda.current_stream()
    K = 1 << a.log_clients
    logs = HH.hierarchy()
    dpf = HH.create_dpf(logs)
    _, _, alphas = HH.client_values(K, seed=0x5B)
    seeds = np.random.default_rng(7).integers(0, 2**64, size=(2 * K, 2), dtype=np.uint64)
    beta = D.to_value(HH.value_type(), HH.BETA)
    b0, b1 = dpf.generate_key_batch(alphas, [beta] * len(logs), root_seeds=seeds, threads=16)
    servers = [HH.Server(dpf, dpf.upload_key_batch(b), 4 * a.top_k + 256, dev) for b in (b0, b1)]
    kernels = {}

    def one_pass(name):
        for srv in servers:
            srv.reset()
        if name == "stream":
            os.environ["DPF_BATCH_SKETCH_FUSED"] = "0"
        flagged = []
        try:
            HH.run(dpf, servers, logs, top_k=a.top_k, keep_cache=True,
                   sketch_seed=None if name == "sum" else 17, flagged=flagged)
        finally:
            os.environ.pop("DPF_BATCH_SKETCH_FUSED", None)
        kernels[name] = H.last_batch_kernel()
        assert all(not bad for _, bad in flagged), "an honest client was flagged"

    variants = ("sum", "fused", "stream")
    for name in variants:
        for _ in range(a.warmup):
            one_pass(name)
    torch.cuda.synchronize()
    sec = {name: [] for name in variants}
    for _ in range(a.reps):
        for name in variants:
            e0, e1 = H.Event(), H.Event()
            e0.record(s)
            one_pass(name)
            e1.record(s)
            torch.cuda.synchronize()
            sec[name].append(e0.elapsed_ms(e1) * 1e-3)
    base = float(np.median(sec["sum"]))
    for name in variants:
        v = sec[name]
        line = {"variant": name, "clients": K, "levels": len(logs), "top_k": a.top_k,
                "weight_rows": 0 if name == "sum" else 2, "reps": len(v),
                "s_median": float(np.median(v)), "s_min": float(np.min(v)),
                "s_max": float(np.max(v)), "ratio_to_sum": float(np.median(v)) / base,
                "last_kernel": kernels[name]}
        out = json.dumps(line)
        print(out, flush=True)
        if a.output:
            with open(a.output, "a") as f:
                f.write(out + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
