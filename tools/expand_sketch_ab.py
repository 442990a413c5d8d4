#!/usr/bin/env python3
"""Same-box, same-session timing of the checked full-domain sum over a key
batch for the heavy-hitters value type Tuple<IntModN<uint32,
2^32 - 5> x 2>.  One session: a warm-up of every path, then `--reps` rounds in
which the three alternate; every timed call ends in a device synchronise;
medians with min and max are reported.

  python tools/expand_sketch_ab.py [--reps 3] [-o profiles/r32/expand_sketch_ab.txt]

  (a) sketch    evaluate_full_domain_sum_sketch_to_device with J = 2 weight rows
  (b) sum       the same with J = 0: (a) - (b) is what the sketches cost
  (c) baseline  the only route before it: a fresh create_batch_evaluation_context
                plus evaluate_until_batch_sketch_to_device(h, [], ...) with sums
Shapes (K, n): (2^16, 12), (2^12, 16), (2^16, 16), (64, 20).  Where the
baseline refuses a shape or runs out of memory (it stores every key's row), its
K is halved until it runs and the line says to what; the comparison is then per
key, and the bytes are compared on that smaller batch.  One JSON line per
shape: the plan, the AES per call from the counts (fused K_padded * 2^walk *
(walk + 2 (2^S - 1) + 2 * 2^S): the tree and the two value hashes per leaf,
keys padded to whole chunks; ideal K * (2 (2^n - 1) + 2 * 2^n); baseline K *
2^(n-2) * (n + 12): n - 2 walked levels, 6 tree and 8 value hashes per four
leaves), milliseconds and G AES/s of each path, the ratios, and whether (a)
and (c) wrote equal bytes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16, 12), (12, 16), (16, 16), (6, 20)]   # (log2 keys, n)


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
    from distributed_point_functions_amd import heavy_hitters as HH
    from distributed_point_functions_amd import hip_abi as H
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

    def stats(xs, aes):
        med = float(np.median(xs))
        return {"ms_median": med * 1e3, "ms_min": float(np.min(xs)) * 1e3,
                "ms_max": float(np.max(xs)) * 1e3, "gaes_per_s": aes / med * 1e-9}

    for log_k, n in shapes:
        N, K = 1 << n, 1 << log_k
        dpf = HH.create_dpf([n])
        rng = np.random.default_rng(n)
        alphas = np.zeros((K, 2), dtype=np.uint64)
        alphas[:, 0] = rng.integers(0, N, size=K, dtype=np.uint64)
        seeds = rng.integers(0, 1 << 63, size=(2 * K, 2), dtype=np.uint64)
        host, _ = dpf.generate_key_batch(alphas, [D.to_value(HH.value_type(), HH.BETA)],
                                         root_seeds=seeds)
        batch = dpf.upload_key_batch(host)
        w = torch.from_numpy(HH.sketch_weights(7, 0, N).view(np.int32)).cuda()
        sum_a = torch.empty((N, 2), dtype=torch.int32, device="cuda")
        sum_b = torch.empty((N, 2), dtype=torch.int32, device="cuda")
        sum_c = torch.empty((N, 2), dtype=torch.int32, device="cuda")
        sk_a = torch.empty((K, 2, 2), dtype=torch.int32, device="cuda")
        sk_c = torch.empty((K, 2, 2), dtype=torch.int32, device="cuda")

        def sketch(b=batch, sk=sk_a):
            dpf.evaluate_full_domain_sum_sketch_to_device(0, b, w, sum_a, sk)

        def plain():
            dpf.evaluate_full_domain_sum_sketch_to_device(0, batch, None, sum_b, None)

        # The baseline on the largest 2^-j of the batch that it takes.
        base_batch, base_k, note = batch, K, None
        while True:
            def baseline(b=base_batch, k=base_k):
                ctx = dpf.create_batch_evaluation_context(b)
                dpf.evaluate_until_batch_sketch_to_device(0, [], ctx, w, sk_c[:k], sums_out=sum_c)
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
                base_batch = dpf.upload_key_batch(host, 0, base_k)
                torch.cuda.empty_cache()

        for _ in range(a.warmup):
            sketch()
            plain()
            if baseline:
                baseline()
        sec = {"sketch": [], "sum": [], "baseline": []}
        for _ in range(a.reps):
            sec["sketch"].append(timed(sketch))
            sec["sum"].append(timed(plain))
            if baseline:
                sec["baseline"].append(timed(baseline))
        pl = H.expand_sketch_plan(K, n, cus)
        S, walk = pl["S"], pl["walk"]
        padded = -(-K // 64) * 64
        aes = padded * pl["subtrees"] * (walk + 2 * ((1 << S) - 1) + 2 * (1 << S))
        ideal = K * (2 * ((1 << n) - 1) + 2 * (1 << n))
        base_aes = base_k * (1 << (n - 2)) * (n + 12)
        line = {"keys": K, "n": n, "plan": pl, "aes_per_call": aes, "aes_ideal": ideal,
                "aes_over_ideal": aes / ideal, "reps": a.reps, "sketch": stats(sec["sketch"], aes),
                "sum": stats(sec["sum"], aes)}
        line["sketch_over_sum"] = line["sketch"]["ms_median"] / line["sum"]["ms_median"]
        line.update({"baseline_keys": base_k, "baseline_cut": base_k != K, "baseline_note": note,
                     "baseline_aes_per_call": base_aes})
        if baseline:
            line["baseline"] = stats(sec["baseline"], base_aes)
            per_key = line["baseline"]["ms_median"] / base_k
            line["baseline_ms_scaled_to_keys"] = per_key * K
            line["baseline_over_sketch"] = per_key * K / line["sketch"]["ms_median"]
            # Equal bytes on the batch the baseline took.
            sketch(base_batch, sk_a[:base_k])
            baseline()
            torch.cuda.synchronize()
            line["equal_bytes"] = bool(torch.equal(sum_a, sum_c) and
                                       torch.equal(sk_a[:base_k], sk_c[:base_k]))
        sketch()
        line["dynamic_chunks"] = H.last_dynamic_chunks()
        torch.cuda.synchronize()
        text = json.dumps(line)
        print(text, flush=True)
        if a.output:
            os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
            with open(a.output, "a") as f:
                f.write(text + "\n")
        del batch, base_batch, sum_a, sum_b, sum_c, sk_a, sk_c, w
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
