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

  python tools/expand_sum_ab.py --type int --bits 8 [-o profiles/r35/expand_sum_packed_ab.txt]

With --type int|xor and --bits 8|16|32|64|128 other than the uint64 default,
the value type is that one and three legs alternate in the session on every
shape:
  (a) packed    evaluate_full_domain_sum_packed_to_device (tree depth n - log2 E)
  (b) baseline  the batched prefix path with sum_over_keys=True on the same
                keys: the only route these types had
  (c) widened   the fused uint64 call at the same K and n: what a user pays who
                widens every key to 64 bits (its own keys, same alphas)
The AES counts of (a) and (c) come from the plan at their own depths; the line
adds (c)'s seconds and AES/s, the AES-count ratio (c)/(a) -- the expectation --
the measured time ratio (c)/(a), the AES/s ratio (a)/(c), each leg's spread
(max - min) / median over the repetitions, and byte-equality of (a) with (b).
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
    ap.add_argument("--type", choices=["int", "xor"], default="int")
    ap.add_argument("--bits", type=int, choices=[8, 16, 32, 64, 128], default=64)
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

    packed = (a.type, a.bits) != ("int", 64)
    if a.type == "int" and a.bits == 128:
        ap.error("additive 128-bit values have no full-domain sum")
    vt = D.xor_wrapper_type(a.bits) if a.type == "xor" else D.integer_type(a.bits)
    log2e = (128 // a.bits).bit_length() - 1

    def make_dpf(n, value_type):
        p = pb.DpfParameters()
        p.log_domain_size = n
        p.value_type.CopyFrom(value_type)
        dpf = D.DistributedPointFunction.create(p)
        dpf.register_value_type(value_type)
        return dpf

    def aes_of(pl, K):
        padded = -(-K // 64) * 64
        S, walk = pl["S"], pl["walk"]
        return padded * pl["subtrees"] * (walk + 2 * ((1 << S) - 1) + (1 << S))

    def spread(v):
        return float((np.max(v) - np.min(v)) / np.median(v))

    for log_k, n in shapes:
        N, K, depth = 1 << n, 1 << log_k, n - log2e
        dpf = make_dpf(n, vt)
        rng = np.random.default_rng(n)
        alphas = np.zeros((K, 2), dtype=np.uint64)
        alphas[:, 0] = rng.integers(0, N, size=K, dtype=np.uint64)
        seeds = rng.integers(0, 1 << 63, size=(2 * K, 2), dtype=np.uint64)
        batch, _ = HG.submit(dpf, alphas, [D.to_value(vt, 1)], seeds)
        out_f = torch.empty(N * a.bits // 64, dtype=torch.int64, device="cuda")
        out_b = torch.empty(N * a.bits // 64, dtype=torch.int64, device="cuda")

        if packed:
            def fused(b=batch):
                dpf.evaluate_full_domain_sum_packed_to_device(b, 0, out_f)
            fold = lambda b: dpf.evaluate_full_domain_sum_packed_to_device(b, 0, out_f)
            # (c): the same bins through keys widened to uint64.
            wide_dpf = make_dpf(n, D.integer_type(64))
            wide_batch, _ = HG.submit(wide_dpf, alphas, [D.to_value(D.integer_type(64), 1)], seeds)
            out_w = torch.empty(N, dtype=torch.int64, device="cuda")

            def widened():
                HG.fold(wide_dpf, wide_batch, out=out_w)
        else:
            def fused(b=batch):
                HG.fold(dpf, b, out=out_f)
            fold = lambda b: HG.fold(dpf, b, out=out_f)
            widened = None

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
            if widened:
                widened()
        sec = {"fused": [], "baseline": [], "widened": []}
        for _ in range(a.reps):
            sec["fused"].append(timed(fused))
            if baseline:
                sec["baseline"].append(timed(baseline))
            if widened:
                sec["widened"].append(timed(widened))
        pl = H.expand_sum_plan(K, depth, cus)
        aes = aes_of(pl, K)
        ideal = K * (2 * ((1 << depth) - 1) + (1 << depth))
        base_aes = base_k * (1 << max(depth - 2, 0)) * (depth + 8) if depth >= 2 else None
        tf = float(np.median(sec["fused"]))
        line = {"type": a.type, "bits": a.bits, "tree_depth": depth, "keys": K, "n": n, "plan": pl, "aes_per_call": aes, "aes_ideal": ideal,
                "aes_over_ideal": aes / ideal, "reps": a.reps, "fused_s_median": tf,
                "fused_s_min": float(np.min(sec["fused"])), "fused_aes_per_s": aes / tf,
                "baseline_keys": base_k, "baseline_cut": base_k != K, "baseline_note": note,
                "baseline_aes_per_call": base_aes}
        if baseline:
            tb = float(np.median(sec["baseline"]))
            # Equal bytes on the batch the baseline took.
            if base_k != K:
                fold(base_batch)
            else:
                fused()
            baseline()
            torch.cuda.synchronize()
            line.update({"baseline_s_median": tb, "baseline_s_min": float(np.min(sec["baseline"])),
                         "baseline_aes_per_s": base_aes / tb if base_aes else None,
                         "baseline_s_scaled_to_keys": tb * K / base_k,
                         "baseline_over_fused": tb * K / base_k / tf,
                         "equal_bytes": bool(torch.equal(out_f, out_b))})
        if widened:
            tw = float(np.median(sec["widened"]))
            wide_aes = aes_of(H.expand_sum_plan(K, n - 1, cus), K)
            line.update({"fused_spread": spread(sec["fused"]),
                         "widened_s_median": tw, "widened_s_min": float(np.min(sec["widened"])),
                         "widened_spread": spread(sec["widened"]),
                         "widened_aes_per_call": wide_aes, "widened_aes_per_s": wide_aes / tw,
                         "aes_count_widened_over_packed": wide_aes / aes,
                         "time_widened_over_packed": tw / tf,
                         "aes_rate_packed_over_widened": (aes / tf) / (wide_aes / tw)})
            if baseline:
                line["baseline_spread"] = spread(sec["baseline"])
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
        if widened:
            del wide_batch, out_w
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
