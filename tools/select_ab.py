#!/usr/bin/env python3
"""Same-box, same-session timing of the bit-selected database fold (DESIGN.md
6b): HIP events around each launch sequence, a warm-up, then `--reps` rounds
in which the variants alternate.  Every width runs as a child process of its
own under a time limit, and a child that fails ends the run.  Random keys and
selection rows: timing only, parity is the tests' job.

  python tools/select_ab.py [--gib 4] [--words 4 32] [-o profiles/r23/select_ab.txt]

Per width W, on a database of `--gib` GiB (2^k records of W uint64 words):
  (a) select/Q     dpf_hip_select_rows alone, Q in {1, 4, 16, 64}
  (b) api/Q        the whole EvaluateSelectToDevice call for the same Q, and
      expand/Q     its expansions alone (Q dpf_hip_expand of the whole domain)
  (c) dot_rows     dpf_hip_dot_rows (XorWrapper<uint128>) on the same bytes
      api_1x16     16 sequential EvaluateSelectToDevice calls of one key
One JSON line per variant: median, min and max ms, database bytes per second
at the median, and ms per query.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12   # achievable HBM rate of the MI355X (float4 copy)
QUERIES = (1, 4, 16, 64)


def child(a):
    import numpy as np
    import torch
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import hip_abi as H
    from distributed_point_functions_amd import proto as pb
    H.load(require_gpu=True)
    dev = torch.device("cuda")
    s = torch.cuda.current_stream()
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    W = a.child
    n = (a.gib << 30) // (8 * W)            # records: a power of two
    depth = n.bit_length() - 1 - 7          # leaf blocks of 128 records
    assert n == 128 << depth

    def rand64(count):
        return torch.randint(-2**63, 2**63 - 1, (count,), dtype=torch.int64, device=dev,
                             generator=g)

    db = rand64(n * W)
    stride = n // 8
    sel = rand64(max(QUERIES) * stride // 8).view(torch.uint8)
    out = torch.empty(max(QUERIES) * W, dtype=torch.int64, device=dev)
    ws = torch.empty(H.select_workspace_bytes(W, max(QUERIES)), dtype=torch.uint8, device=dev)

    variants, shapes = {}, {}
    for q in QUERIES:
        variants[f"select/{q}"] = (
            lambda q=q: H.select_rows(n, W, q, sel, stride, db, workspace=ws, out=out), q)

    # (c) dot_rows on equal bytes: n / 2 records of W uint128 words.
    desc = H.value_desc([(H.LEAF_XOR, 128, 0)], True, 1, 1)
    y = rand64(n)
    dws = torch.empty(H.dot_workspace_bytes(desc, W), dtype=torch.uint8, device=dev)
    dres = torch.empty(W * 16, dtype=torch.uint8, device=dev)
    variants["dot_rows"] = (lambda: H.dot_rows(n // 2, W, desc, y, db, workspace=dws, out=dres), 1)

    # (b) the API, and its expansions alone.
    vt = D.xor_wrapper_type(128)
    p = pb.DpfParameters(log_domain_size=depth)
    p.value_type.CopyFrom(vt)
    dpf = D.DistributedPointFunction.create(p)
    dpf.register_value_type(vt)
    rng = np.random.default_rng(11)
    keys = [dpf.generate_keys_incremental(int(rng.integers(0, 1 << depth)),
                                          [D.to_value(vt, 1 << int(rng.integers(0, 128)))])[0]
            for _ in range(max(QUERIES))]
    share = torch.empty(n // 8, dtype=torch.uint8, device=dev)

    def expansions(q):
        for k in keys[:q]:
            dpf.evaluate_shard_to_device(0, 0, 1, dpf.create_evaluation_context(k), share)

    for q in QUERIES:
        variants[f"api/{q}"] = (
            lambda q=q: dpf.evaluate_select_to_device(keys[:q], 0, db, W, out), q)
        variants[f"expand/{q}"] = (lambda q=q: expansions(q), q)

    def sequential():
        for k in keys[:16]:
            dpf.evaluate_select_to_device([k], 0, db, W, out)
    variants["api_1x16"] = (sequential, 16)

    for name, (fn, _) in variants.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        if name.startswith(("select", "api")):
            shapes[name] = list(H.last_select_shape())
    ms = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, (fn, _) in variants.items():
            e0, e1 = H.Event(), H.Event()
            e0.record(s)
            fn()
            e1.record(s)
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_ms(e1))
    for name, v in ms.items():
        q = variants[name][1]
        med = float(np.median(v))
        passes = 16 if name == "api_1x16" else shapes.get(name, [0, 1, 0])[1]
        line = {"variant": name, "record_words": W, "records": n, "db_bytes": n * W * 8,
                "reps": len(v), "ms_median": med, "ms_min": float(np.min(v)),
                "ms_max": float(np.max(v)), "ms_per_query": med / q}
        if not name.startswith("expand"):
            line["db_passes"] = passes
            line["db_tbytes_per_s"] = passes * n * W * 8 / (med * 1e-3) / 1e12
            line["ms_at_hbm_rate"] = passes * n * W * 8 / HBM_BYTES_PER_S * 1e3
        if name in shapes:
            line["select_shape"] = shapes[name]
        print(json.dumps(line), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4, help="database size (a power of two)")
    ap.add_argument("--words", type=int, nargs="+", default=[4, 32],
                    help="record widths (powers of two)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per width")
    ap.add_argument("-o", "--output", help="also append the lines to this file")
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for w in a.words:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__),
               "--child", str(w), "--gib", str(a.gib), "--reps", str(a.reps),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr)
        if a.output:
            with open(a.output, "a") as f:
                f.write(r.stdout)
        if r.returncode != 0:
            print(f"select_ab: W = {w} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
