#!/usr/bin/env python3
"""Same-box, same-session timing of the batched private table lookup
(DESIGN.md 6f): the fused call against the composition the engine offered
before it, for uint64 values.  One session: a warm-up of both paths, then
`--reps` rounds in which the two alternate; every timed call ends in a device
synchronise; medians are reported.

  python tools/lookup_ab.py [--reps 3] [-o profiles/r30/lookup_ab.txt]

  (a) fused        evaluate_lookup_batch_to_device: one launch, no share vector
  (b) composition  evaluate_until_batch_to_device storing [key][element], then
                   a torch gather-and-reduce with the same rotation,
                   out[k][w] = sum_i y[k][i] * T[(i + s_k) mod N][w], taken in
                   slices of keys whose gathered rows stay below 1 GiB
Shapes: K = 2^16 at n = 8 and 12, K = 2^12 at n = 16, W = 1 and 4.  K is halved
while the composition's share vector (K * 2^n * 8 bytes) would exceed a quarter
of the free device memory, and the line says so.  One JSON line per shape: the
plan, the AES per launch from the plan's counts and their ratio to the ideal
2 (2^D - 1) + 2^D per key, seconds and AES/s of both paths, their ratio, and
whether both produced equal bytes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16, 8), (16, 12), (12, 16)]   # (log2 keys, n)


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
    from distributed_point_functions_amd import lookup as LK
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
        N = 1 << n
        free, _ = torch.cuda.mem_get_info()
        cut = 0
        while (1 << (log_k - cut)) * N * 8 > free // 4:
            cut += 1
        K = 1 << (log_k - cut)
        p = pb.DpfParameters()
        p.log_domain_size = n
        p.value_type.CopyFrom(D.integer_type(64))
        dpf = D.DistributedPointFunction.create(p)
        rng = np.random.default_rng(n)
        masks = np.zeros((K, 2), dtype=np.uint64)
        masks[:, 0] = rng.integers(0, N, size=K, dtype=np.uint64)
        seeds = rng.integers(0, 1 << 63, size=(2 * K, 2), dtype=np.uint64)
        batch, _ = LK.deal(dpf, masks, [D.to_value(D.integer_type(64), 1)], seeds)
        offsets = torch.from_numpy(rng.integers(0, 1 << 63, size=K, dtype=np.int64)).cuda()
        ctx = dpf.create_batch_evaluation_context(batch)
        shares = torch.empty((K, N), dtype=torch.int64, device="cuda")
        ar = torch.arange(N, dtype=torch.int64, device="cuda")
        for W in (1, 4):
            table = torch.from_numpy(
                rng.integers(-(1 << 63), 1 << 63, size=(N, W), dtype=np.int64)).cuda()
            out_f = torch.empty((K, W), dtype=torch.int64, device="cuda")
            out_c = torch.empty((K, W), dtype=torch.int64, device="cuda")
            step = max(1, min(K, (1 << 30) // (N * W * 8)))

            def fused():
                LK.evaluate(dpf, batch, offsets, table, W, out=out_f)

            def composition():
                ctx.reset()
                dpf.evaluate_until_batch_to_device(0, [], ctx, shares)
                for k0 in range(0, K, step):
                    idx = (ar[None, :] + offsets[k0:k0 + step, None]) & (N - 1)
                    out_c[k0:k0 + step] = (shares[k0:k0 + step, :, None] * table[idx]).sum(1)

            for _ in range(a.warmup):
                fused()
                composition()
            sec = {"fused": [], "composition": []}
            for _ in range(a.reps):
                sec["fused"].append(timed(fused))
                sec["composition"].append(timed(composition))
            pl = H.lookup_plan(K, n - 1, W, cus)
            depth, S, walk = n - 1, pl["S"], pl["walk"]
            aes = K * pl["items_per_key"] * (walk + 2 * ((1 << S) - 1) + (1 << S))
            ideal = K * (2 * ((1 << depth) - 1) + (1 << depth))
            tf, tc = float(np.median(sec["fused"])), float(np.median(sec["composition"]))
            line = {"keys": K, "keys_cut_by_log2": cut, "n": n, "table_words": W, "plan": pl,
                    "aes_per_launch": aes, "aes_over_ideal": aes / ideal, "reps": a.reps,
                    "fused_s_median": tf, "fused_s_min": float(np.min(sec["fused"])),
                    "fused_aes_per_s": aes / tf,
                    "composition_s_median": tc, "composition_s_min": float(np.min(sec["composition"])),
                    "composition_aes_per_s": ideal / tc, "composition_over_fused": tc / tf,
                    "equal_bytes": bool(torch.equal(out_f, out_c)),
                    "dynamic_chunks": None}
            fused()
            line["dynamic_chunks"] = H.last_dynamic_chunks()
            torch.cuda.synchronize()
            text = json.dumps(line)
            print(text, flush=True)
            if a.output:
                os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
                with open(a.output, "a") as f:
                    f.write(text + "\n")
        del shares, ctx, batch
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
