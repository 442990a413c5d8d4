#!/usr/bin/env python3
"""Same-box, same-session timing of full-domain DCF evaluation:
wall-clock seconds, the device idle before and after each timed call, of

  (a) full     evaluate_full_domain_to_device (dpf_hip_dcf_expand: one
               depth-first walk of the key's tree)
  (b) points   evaluate_batch_to_device at all 2^n points, shared by the keys
               (dcf_fast_kernel: one root-to-leaf walk per point) -- the only
               way to the same vector before (a) existed, hence the baseline
  (c) dpf      a uint64 DistributedPointFunction's evaluate_shard_to_device of
               the same 2^n outputs (the DPF's full-domain path)

for a uint64 DCF of one key at n = 16, 20, 24 and 28, and (a) and (b) for a
batch of 2^12 keys at n = 12.  A warm-up, then `--reps` rounds in which the
calls alternate; medians.  Each line carries the AES calls of one launch by
the operation counts -- (a) 2^(n+1) - 3, (b) (2n - 1) 2^n, (c) 3 2^(n-1) - 2 per
key -- the rates they give, and whether (a) and (b) wrote the same bytes.

  python tools/dcf_expand_ab.py [--reps 3] [--cases 16,20,24,28,batch] [-o profiles/r29/dcf_expand_ab.txt]

One JSON line per case.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="16,20,24,28,batch",
                    help="comma-separated: log domain sizes of the one-key cases, and `batch`")
    ap.add_argument("-o", "--output", help="also append the lines to this file")
    a = ap.parse_args()

    import numpy as np
    import torch
    from distributed_point_functions_amd import dcf as C
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import hip_abi as H
    from distributed_point_functions_amd import proto as pb
    H.load(require_gpu=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def make_dcf(n):
        p = pb.DcfParameters()
        p.parameters.log_domain_size = n
        p.parameters.value_type.CopyFrom(D.integer_type(64))
        return C.DistributedComparisonFunction.create(p)

    def all_points(n):
        pts = torch.zeros((1 << n, 2), dtype=torch.int64, device="cuda")
        pts[:, 0] = torch.arange(1 << n, dtype=torch.int64, device="cuda")
        return pts

    def run(name, n, keys, calls, aes, extra):
        for _ in range(a.warmup):
            for f in calls.values():
                f()
        sec = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                sec[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in sec.items()}
        line = {"case": name, "log_domain_size": n, "keys": keys, "reps": a.reps}
        for k in calls:
            line[f"{k}_s"] = med[k]
            line[f"{k}_aes"] = aes[k]
            line[f"{k}_aes_per_s"] = aes[k] / med[k]
        line["points_over_full"] = med["points"] / med["full"]
        line["aes_ratio_points_over_full"] = aes["points"] / aes["full"]
        if "dpf" in med:
            line["full_over_dpf"] = med["full"] / med["dpf"]
        line.update(extra())
        line["plan"] = H.dcf_expand_plan(keys, n, 0, cus)
        line["gpu"] = torch.cuda.get_device_name(0)
        out = json.dumps(line)
        print(out, flush=True)
        if a.output:
            with open(a.output, "a") as f:
                f.write(out + "\n")

    def one_key(n):
        dcf = make_dcf(n)
        key = dcf.generate_keys((5 << n) // 7, 42, seed_0=1, seed_1=2)[0]
        dev = dcf.upload_key_batch(dcf.make_key_batch([key]))
        pts = all_points(n)
        out_full = torch.empty(1 << n, dtype=torch.int64, device="cuda")
        out_pts = torch.empty(1 << n, dtype=torch.int64, device="cuda")
        p = pb.DpfParameters()
        p.log_domain_size = n
        p.value_type.CopyFrom(D.integer_type(64))
        dpf = D.DistributedPointFunction.create(p)
        dkey = dpf.generate_keys_incremental((5 << n) // 7, [D.to_value(D.integer_type(64), 42)],
                                             seeds=(1, 2))[0]
        out_dpf = torch.empty(1 << n, dtype=torch.int64, device="cuda")
        calls = {
            "full": lambda: dcf.evaluate_full_domain_to_device(key, out_full),
            "points": lambda: dcf.evaluate_batch_to_device(dev, pts, 1 << n, out_pts,
                                                           shared_points=True),
            "dpf": lambda: dpf.evaluate_shard_to_device(0, 0, 1, dpf.create_evaluation_context(dkey),
                                                        out_dpf),
        }
        aes = {"full": (2 << n) - 3, "points": (2 * n - 1) << n, "dpf": 3 * (1 << n) // 2 - 2}
        run("dcf_u64_one_key", n, 1, calls, aes,
            lambda: {"full_equals_points": bool(torch.equal(out_full, out_pts))})

    def batch():
        n, keys = 12, 1 << 12
        dcf = make_dcf(n)
        rng = np.random.default_rng(3)
        alphas = rng.integers(0, 1 << n, size=(keys, 2), dtype=np.uint64)
        alphas[:, 1] = 0
        seeds = rng.integers(0, 2**64, size=(2 * keys, 2), dtype=np.uint64)
        dev = dcf.generate_key_batch_to_device(alphas, [42], root_seeds=seeds)[0]
        pts = all_points(n)
        out_full = torch.empty(keys << n, dtype=torch.int64, device="cuda")
        out_pts = torch.empty(keys << n, dtype=torch.int64, device="cuda")
        calls = {
            "full": lambda: dcf.evaluate_full_domain_batch_to_device(dev, out_full),
            "points": lambda: dcf.evaluate_batch_to_device(dev, pts, 1 << n, out_pts,
                                                           shared_points=True),
        }
        aes = {"full": keys * ((2 << n) - 3), "points": keys * ((2 * n - 1) << n)}
        run("dcf_u64_key_batch", n, keys, calls, aes,
            lambda: {"full_equals_points": bool(torch.equal(out_full, out_pts))})

    for c in a.cases.split(","):
        if c == "batch":
            batch()
        else:
            one_key(int(c))
    return 0


if __name__ == "__main__":
    sys.exit(main())
