#!/usr/bin/env python3
"""Same-box, same-session timing of batched key generation:
wall-clock seconds, the device idle before and after each timed call, of

  (a) host    generate_key_batch on 16 host threads, then the upload of both
              parties' batches
  (b) device  generate_key_batch_to_device (root seeds drawn and uploaded, the
              key generation kernel, the device-to-device copy of the
              correction words)
  (c) download  both device batches back to host memory, reported apart

for three cases: 2^16 DCF keys at n = 64 (uint64), 2^20 single-level DPF keys
at log_domain_size 128 (uint64), and the heavy-hitters hierarchy (a tuple of
IntModN, which takes the host fallback).  A warm-up, then `--reps` rounds in
which (a) and (b) alternate.  Timing only: parity is the tests' job.  The root
seeds are given, so that both paths generate the same keys.

  python tools/keygen_ab.py [--reps 3] [--scale 0] [--cases dcf,dpf,hh] [-o profiles/r26/keygen_ab.txt]

One JSON line per case.  --scale s divides every key count by 2^s (smoke runs).
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
    ap.add_argument("--scale", type=int, default=0)
    ap.add_argument("--cases", default="dcf,dpf,hh", help="comma-separated: dcf, dpf, hh")
    ap.add_argument("-o", "--output", help="also append the lines to this file")
    a = ap.parse_args()

    import numpy as np
    import torch
    from distributed_point_functions_amd import dcf as C
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import heavy_hitters as HH
    from distributed_point_functions_amd import hip_abi as H
    from distributed_point_functions_amd import proto as pb
    H.load(require_gpu=True)
    rng = np.random.default_rng(11)

    def u128(n, bits):
        x = rng.integers(0, 2**64, size=(n, 2), dtype=np.uint64)
        if bits <= 64:
            x[:, 1] = 0
            if bits < 64:
                x[:, 0] &= np.uint64((1 << bits) - 1)
        elif bits < 128:
            x[:, 1] &= np.uint64((1 << (bits - 64)) - 1)
        return x

    def dcf_case():
        K = (1 << 16) >> a.scale
        p = pb.DcfParameters()
        p.parameters.log_domain_size = 64
        p.parameters.value_type.CopyFrom(D.integer_type(64))
        dcf = C.DistributedComparisonFunction.create(p)
        alphas, seeds = u128(K, 64), u128(2 * K, 128)
        return ("dcf_n64_u64", K, dcf, dcf.generates_keys_on_device(),
                lambda: dcf.generate_key_batch(alphas, [42], root_seeds=seeds, threads=16),
                lambda: dcf.generate_key_batch_to_device(alphas, [42], root_seeds=seeds))

    def dpf_case():
        K = (1 << 20) >> a.scale
        p = pb.DpfParameters()
        p.log_domain_size = 128
        p.value_type.CopyFrom(D.integer_type(64))
        dpf = D.DistributedPointFunction.create(p)
        alphas, seeds = u128(K, 128), u128(2 * K, 128)
        beta = [D.to_value(D.integer_type(64), 42)]
        return ("dpf_log128_u64", K, dpf, dpf.generates_keys_on_device(),
                lambda: dpf.generate_key_batch(alphas, beta, root_seeds=seeds, threads=16),
                lambda: dpf.generate_key_batch_to_device(alphas, beta, root_seeds=seeds))

    def hh_case():
        K = (1 << 18) >> a.scale
        logs = HH.hierarchy()
        dpf = HH.create_dpf(logs)
        _, _, alphas = HH.client_values(K, seed=0x5B)   # uint64 (K, 2) already
        seeds = u128(2 * K, 128)
        beta = [D.to_value(HH.value_type(), HH.BETA)] * len(logs)
        return ("heavy_hitters_fallback", K, dpf, dpf.generates_keys_on_device(),
                lambda: dpf.generate_key_batch(alphas, beta, root_seeds=seeds, threads=16),
                lambda: dpf.generate_key_batch_to_device(alphas, beta, root_seeds=seeds))

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    cases = {"dcf": dcf_case, "dpf": dpf_case, "hh": hh_case}
    for make in (cases[c] for c in a.cases.split(",")):
        name, K, obj, on_device, host_gen, device_gen = make()

        def host():
            b0, b1 = host_gen()
            return obj.upload_key_batch(b0), obj.upload_key_batch(b1)

        for _ in range(a.warmup):
            host()
            device_gen()
        sec = {"host": [], "host_generate": [], "device": [], "download": []}
        for _ in range(a.reps):
            t_gen, batches = timed(host_gen)
            t_up, _ = timed(lambda: [obj.upload_key_batch(b) for b in batches])
            sec["host_generate"].append(t_gen)
            sec["host"].append(t_gen + t_up)
            del batches
            t_dev, dev = timed(device_gen)
            sec["device"].append(t_dev)
            t_down, _ = timed(lambda: [obj.download_key_batch(d) for d in dev])
            sec["download"].append(t_down)
            del dev
        med = {k: float(np.median(v)) for k, v in sec.items()}
        line = {"case": name, "key_pairs": K, "on_device": bool(on_device), "reps": a.reps,
                "host_16_threads_then_upload_s": med["host"],
                "host_generate_s": med["host_generate"],
                "generate_to_device_s": med["device"], "download_s": med["download"],
                "host_over_device": med["host"] / med["device"],
                "device_key_pairs_per_s": K / med["device"],
                "gpu": torch.cuda.get_device_name(0)}
        out = json.dumps(line)
        print(out, flush=True)
        if a.output:
            with open(a.output, "a") as f:
                f.write(out + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
