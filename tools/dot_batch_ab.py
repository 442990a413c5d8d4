#!/usr/bin/env python3
"""Same-box, same-session timing of the batched database fold:
HIP events around each launch sequence, a warm-up, then `--reps` rounds in
which the variants alternate; every timed call ends in a synchronise.  Every
width runs as a child process of its own under a time limit, and a child that
fails ends the run.  Random keys, shares and records: timing only, parity is
the tests' job.

  python tools/dot_batch_ab.py [--gib 4] [--words 32 4] [-o profiles/r33/dot_batch_ab.txt]

Per width W, on a uint64_t database of `--gib` GiB (2^k records of W words)
and Q in {1, 4, 16, 64}:
  (a) rows_batch/Q  dpf_hip_dot_rows_batch alone, on the first 2^--kernel-log
                    records at most (Q share rows of 8 bytes per record have
                    to fit beside the database)
  (b) api/Q         the whole EvaluateDotBatchToDevice call (api_t<T>/Q: with
                    the host tile `--tiles` names, DPF_DOT_BATCH_TILE=T)
  (c) seq/Q         Q sequential EvaluateDotToDevice calls, one key each
  (d) expand/Q      the Q expansions alone (Q full-domain dpf_hip_expand)
One JSON line per variant: median, min and max ms, ms per query and, for (a)
to (c), the database bytes read per second at the median.  A last line per Q
gives seq/Q over api/Q at the medians and whether the rounds' ranges are
disjoint (the slowest api round against the fastest seq round).
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


def host_tile(W):
    """Keys EvaluateDotBatchToDevice hands the kernel at a time."""
    return 8 if W >= 16 else 4


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
    log_n = n.bit_length() - 1
    assert n == 1 << log_n
    nk = min(n, 1 << a.kernel_log)          # records of the kernel-alone runs
    Qmax = max(QUERIES)

    def rand64(count):
        return torch.randint(-2**63, 2**63 - 1, (count,), dtype=torch.int64, device=dev,
                             generator=g)

    db = rand64(n * W)
    y = rand64(Qmax * nk)
    out = torch.empty(Qmax * W, dtype=torch.int64, device=dev)
    desc = H.value_desc([(H.LEAF_INT, 64, 0)], True, 2, 1)
    ws = torch.empty(H.dot_batch_workspace_bytes(desc, W, Qmax), dtype=torch.uint8, device=dev)

    variants, shapes, rows = {}, {}, {}
    for q in QUERIES:
        variants[f"rows_batch/{q}"] = (
            lambda q=q: H.dot_rows_batch(nk, W, q, desc, y, nk * 8, db, workspace=ws, out=out), q)
        rows[f"rows_batch/{q}"] = nk

    vt = D.integer_type(64)
    p = pb.DpfParameters(log_domain_size=log_n)
    p.value_type.CopyFrom(vt)
    dpf = D.DistributedPointFunction.create(p)
    dpf.register_value_type(vt)
    rng = np.random.default_rng(11)
    keys = [dpf.generate_keys_incremental(
        int(rng.integers(0, n)), [D.to_value(vt, int(rng.integers(1, 2**63)))])[0]
        for _ in range(Qmax)]
    share = torch.empty(n, dtype=torch.int64, device=dev)

    def sequential(q):
        for i, k in enumerate(keys[:q]):
            dpf.evaluate_dot_to_device(k, 0, db, W, out[i * W:(i + 1) * W])

    def expansions(q):
        for k in keys[:q]:
            dpf.evaluate_shard_to_device(0, 0, 1, dpf.create_evaluation_context(k), share)

    def tiled(q, tile):
        os.environ["DPF_DOT_BATCH_TILE"] = str(tile)
        try:
            dpf.evaluate_dot_batch_to_device(keys[:q], 0, db, W, out)
        finally:
            del os.environ["DPF_DOT_BATCH_TILE"]

    passes = {}
    for q in QUERIES:
        variants[f"api/{q}"] = (
            lambda q=q: dpf.evaluate_dot_batch_to_device(keys[:q], 0, db, W, out), q)
        variants[f"seq/{q}"] = (lambda q=q: sequential(q), q)
        variants[f"expand/{q}"] = (lambda q=q: expansions(q), q)
        rows[f"api/{q}"] = rows[f"seq/{q}"] = n
        passes[f"api/{q}"], passes[f"seq/{q}"] = -(-q // host_tile(W)), q
        for t in a.tiles:
            if t < q:
                variants[f"api_t{t}/{q}"] = (lambda q=q, t=t: tiled(q, t), q)
                rows[f"api_t{t}/{q}"], passes[f"api_t{t}/{q}"] = n, -(-q // t)

    for name, (fn, _) in variants.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        if name.startswith("rows_batch"):
            shapes[name] = list(H.last_dot_batch_shape())
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
        line = {"variant": name, "record_words": W, "records": rows.get(name, n), "reps": len(v),
                "ms_median": med, "ms_min": float(np.min(v)), "ms_max": float(np.max(v)),
                "ms_per_query": med / q}
        if name in rows:
            npass = passes[name] if name in passes else shapes[name][1]
            nbytes = rows[name] * W * 8
            line["db_bytes"] = nbytes
            line["db_passes"] = npass
            line["db_tbytes_per_s"] = npass * nbytes / (med * 1e-3) / 1e12
            line["ms_at_hbm_rate"] = npass * nbytes / HBM_BYTES_PER_S * 1e3
        if name in shapes:
            line["batch_shape"] = shapes[name]
        print(json.dumps(line), flush=True)
    for q in QUERIES:
        api, seq = ms[f"api/{q}"], ms[f"seq/{q}"]
        print(json.dumps({"variant": f"seq_over_api/{q}", "record_words": W,
                          "ratio_of_medians": float(np.median(seq) / np.median(api)),
                          "api_ms_range": [float(np.min(api)), float(np.max(api))],
                          "seq_ms_range": [float(np.min(seq)), float(np.max(seq))],
                          "ranges_disjoint": bool(np.max(api) < np.min(seq))}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4, help="database size (a power of two)")
    ap.add_argument("--words", type=int, nargs="+", default=[32, 4],
                    help="record widths (powers of two)")
    ap.add_argument("--kernel-log", type=int, default=25,
                    help="log2 of the records of the kernel-alone runs, at most")
    ap.add_argument("--tiles", type=int, nargs="*", default=[],
                    help="also time the API with these host tiles (DPF_DOT_BATCH_TILE)")
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
               "--warmup", str(a.warmup), "--kernel-log", str(a.kernel_log),
               "--tiles", *[str(t) for t in a.tiles]]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr)
        if a.output:
            with open(a.output, "a") as f:
                f.write(r.stdout)
        if r.returncode != 0:
            print(f"dot_batch_ab: W = {w} ended with status {r.returncode}; stopping",
                  file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
