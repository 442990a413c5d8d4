#!/usr/bin/env python3
"""Same-box, same-session timing of the fused full-domain sum over a key batch
(DESIGN.md 6g): the fused call against the only route the engine offered
before it, for uint64 values.  One session: a warm-up of both paths, then
`--reps` rounds in which the two alternate; every timed call ends in a device
synchronise; medians are reported.

  python tools/expand_sum_ab.py [--reps 3] [-o profiles/r31/expand_sum_ab.txt]

  (a) fused     evaluate_full_domain_sum_to_device: a table kernel and one
                launch, no share vector, no context
  (b) baseline  a fresh create_batch_evaluation_context plus
                evaluate_until_batch_to_device(h, [], ctx, out, sum_over_keys=True)
Shapes (K, n): (2^16, 12), (2^16, 16), (2^20, 10), (2^12, 20), (64, 24).  Where
the baseline refuses a shape or runs out of memory, its K is halved until it
runs and the line says to what; the bytes are then compared on that smaller
batch.  One JSON line per shape: the plan, the AES per call from the counts
(fused K_padded * 2^walk * (walk + 2 (2^S - 1) + 2^S) with the keys padded to
whole chunks, ideal K * (2 (2^D - 1) + 2^D), baseline K * 2^(D-2) * (D + 8)),
seconds and AES/s of both paths, their ratio, and whether both wrote equal
bytes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16, 12), (16, 16), (20, 10), (12, 20), (6, 24)]   # (log2 keys, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", help="comma-separated logK:n pairs instead of the default shapes")
    ap.add_argument("-o", "--output", help="also append the lines to this file")
    a = ap.parse_args()

    import numpy as np
    import torch
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import hip_abi as H
    from distributed_point_functions_amd import histogram as HG
    from distributed_point_functions_amd import proto as pb
    H.load(require_gpu=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = SHAPES
    if a.shapes:
        shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    for log_k, n in shapes:
        N, K, depth = 1 << n, 1 << log_k, n - 1
        p = pb.DpfParameters()
        p.log_domain_size = n
        p.value_type.CopyFrom(D.integer_type(64))
        dpf = D.DistributedPointFunction.create(p)
        rng = np.random.default_rng(n)
        alphas = np.zeros((K, 2), dtype=np.uint64)
        alphas[:, 0] = rng.integers(0, N, size=K, dtype=np.uint64)
        seeds = rng.integers(0, 1 << 63, size=(2 * K, 2), dtype=np.uint64)
        batch, _ = HG.submit(dpf, alphas, [D.to_value(D.integer_type(64), 1)], seeds)
        out_f = torch.empty(N, dtype=torch.int64, device="cuda")
        out_b = torch.empty(N, dtype=torch.int64, device="cuda")

        def fused(b=batch):
            HG.fold(dpf, b, out=out_f)

        # The baseline on the largest 2^-j of the batch that it takes.
        host = None
        base_batch, base_k, note = batch, K, None
        while True:
            def baseline(b=base_batch):
                ctx = dpf.create_batch_evaluation_context(b)
                dpf.evaluate_until_batch_to_device(0, [], ctx, out_b, sum_over_keys=True)
            try:
                baseline()
                torch.cuda.synchronize()
                break
            except (D.DpfStatusError, RuntimeError) as e:
                note = str(e)[:120]
                if base_k == 1:
                    baseline = None
                    break
                base_k //= 2
                if host is None:
                    host = dpf.download_key_batch(batch)
                base_batch = dpf.upload_key_batch(host, 0, base_k)
                torch.cuda.empty_cache()

        for _ in range(a.warmup):
            fused()
            if baseline:
                baseline()
        sec = {"fused": [], "baseline": []}
        for _ in range(a.reps):
            sec["fused"].append(timed(fused))
            if baseline:
                sec["baseline"].append(timed(baseline))
        pl = H.expand_sum_plan(K, depth, cus)
        S, walk = pl["S"], pl["walk"]
        padded = -(-K // 64) * 64
        aes = padded * pl["subtrees"] * (walk + 2 * ((1 << S) - 1) + (1 << S))
        ideal = K * (2 * ((1 << depth) - 1) + (1 << depth))
        base_aes = base_k * (1 << max(depth - 2, 0)) * (depth + 8) if depth >= 2 else None
        tf = float(np.median(sec["fused"]))
        line = {"keys": K, "n": n, "plan": pl, "aes_per_call": aes, "aes_ideal": ideal,
                "aes_over_ideal": aes / ideal, "reps": a.reps, "fused_s_median": tf,
                "fused_s_min": float(np.min(sec["fused"])), "fused_aes_per_s": aes / tf,
                "baseline_keys": base_k, "baseline_cut": base_k != K, "baseline_note": note,
                "baseline_aes_per_call": base_aes}
        if baseline:
            tb = float(np.median(sec["baseline"]))
            # Equal bytes on the batch the baseline took.
            if base_k != K:
                HG.fold(dpf, base_batch, out=out_f)
            else:
                fused()
            baseline()
            torch.cuda.synchronize()
            line.update({"baseline_s_median": tb, "baseline_s_min": float(np.min(sec["baseline"])),
                         "baseline_aes_per_s": base_aes / tb if base_aes else None,
                         "baseline_s_scaled_to_keys": tb * K / base_k,
                         "baseline_over_fused": tb * K / base_k / tf,
                         "equal_bytes": bool(torch.equal(out_f, out_b))})
        fused()
        line["dynamic_chunks"] = H.last_dynamic_chunks()
        torch.cuda.synchronize()
        text = json.dumps(line)
        print(text, flush=True)
        if a.output:
            os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
            with open(a.output, "a") as f:
                f.write(text + "\n")
        del batch, base_batch, out_f, out_b
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
