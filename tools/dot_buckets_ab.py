#!/usr/bin/env python3
"""Same-box, same-session timing of multi-query PIR over a bucketed database
(DESIGN.md 6j): HIP events around each launch sequence, a warm-up, then
`--reps` rounds in which the variants alternate; every timed call ends in a
synchronise.  Every part runs as a child process of its own under a time
limit, and a child that fails ends the run.  Where two paths are compared they
are first checked to produce equal bytes.

  python tools/dot_buckets_ab.py [--parts gate protocol expand fold] [-o profiles/r34/dot_buckets_ab.txt]

  gate      uint64_t, B = 96 buckets of 2^n records of W words, one key per
            bucket, n in {12, 16, 18}, W in {4, 32}:
              (a) buckets  one EvaluateDotBucketsToDevice call
              (b) per_bucket  one EvaluateDotBatchToDevice call per bucket on
                  that bucket's slice
            and (b) over (a) at the medians with whether the rounds' ranges
            are disjoint (the slowest (a) round against the fastest (b) round).
  protocol  64 queries against R = 2^22 records of 32 words: pir.answer on
            the plain database against pir.answer_buckets on
            BucketLayout(R, 96, seed).encode(db); the encoded size.
  expand    dpf_hip_expand_rows alone at (K, n) = (2^16, 12), (2^12, 16),
            (96, 16): G AES/s by the plan's AES count, and the plan's AES /
            ideal.
  fold      dpf_hip_dot_buckets alone, B = 96, N = 2^16, W = 32, one key per
            bucket: TB/s of database read.
One JSON line per variant: median, min and max ms.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 96


def _timed(variants, a):
    """{name: [ms per round]}: warm-up, then rounds in which the variants alternate."""
    import torch
    from distributed_point_functions_amd import hip_abi as H
    s = torch.cuda.current_stream()
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, fn in variants.items():
            e0, e1 = H.Event(), H.Event()
            e0.record(s)
            fn()
            e1.record(s)
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_ms(e1))
    return ms


def _line(name, v, **more):
    import numpy as np
    line = {"variant": name, "reps": len(v), "ms_median": float(np.median(v)),
            "ms_min": float(np.min(v)), "ms_max": float(np.max(v))}
    line.update(more)
    print(json.dumps(line), flush=True)


def _ratio(name, slow, fast, **more):
    import numpy as np
    print(json.dumps(dict(variant=name, ratio_of_medians=float(np.median(slow) / np.median(fast)),
                          fast_ms_range=[float(np.min(fast)), float(np.max(fast))],
                          slow_ms_range=[float(np.min(slow)), float(np.max(slow))],
                          ranges_disjoint=bool(np.max(fast) < np.min(slow)), **more)), flush=True)


def _make_dpf(log_n):
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import proto as pb
    vt = D.integer_type(64)
    p = pb.DpfParameters(log_domain_size=log_n)
    p.value_type.CopyFrom(vt)
    dpf = D.DistributedPointFunction.create(p)
    dpf.register_value_type(vt)
    return dpf, vt


def _rand64(count, g):
    import torch
    return torch.randint(-2**63, 2**63 - 1, (count,), dtype=torch.int64, device="cuda", generator=g)


def _setup():
    import torch
    from distributed_point_functions_amd import hip_abi as H
    H.load(require_gpu=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    return g


def part_gate(a):
    import numpy as np
    import torch
    from distributed_point_functions_amd import dpf as D
    g = _setup()
    rng = np.random.default_rng(11)
    for n in (12, 16, 18):
        dpf, vt = _make_dpf(n)
        N = 1 << n
        alphas = [int(x) for x in rng.integers(0, N, size=B)]
        host = dpf.generate_key_batch(alphas, [D.to_value(vt, 12345)])[0]
        dev = dpf.upload_key_batch(host)
        keys = [dpf.key_from_batch(host, k) for k in range(B)]
        begin = list(range(B + 1))
        for W in (4, 32):
            db = _rand64(B * N * W, g)
            slices = [db[b * N * W:(b + 1) * N * W] for b in range(B)]
            out_a = torch.empty(B * W, dtype=torch.int64, device="cuda")
            out_b = torch.empty(B * W, dtype=torch.int64, device="cuda")

            def buckets():
                dpf.evaluate_dot_buckets_to_device(dev, 0, begin, db, W, out_a)

            def per_bucket():
                for b in range(B):
                    dpf.evaluate_dot_batch_to_device(keys[b:b + 1], 0, slices[b], W,
                                                     out_b[b * W:(b + 1) * W])

            buckets()
            per_bucket()
            torch.cuda.synchronize()
            assert torch.equal(out_a, out_b), "the two paths differ"
            ms = _timed({"buckets": buckets, "per_bucket": per_bucket}, a)
            shape = dict(part="gate", buckets=B, log_bucket_size=n, record_words=W)
            for name, v in ms.items():
                _line(name, v, db_bytes=B * N * W * 8, **shape)
            _ratio("per_bucket_over_buckets", ms["per_bucket"], ms["buckets"], **shape)
            del db, slices
    return 0


def part_protocol(a):
    import numpy as np
    import torch
    from distributed_point_functions_amd import pir
    g = _setup()
    log_r, W, Q, seed = 22, 32, 64, 5
    R = 1 << log_r
    layout = pir.BucketLayout(R, B, seed)
    n = layout.log_bucket_size
    db = _rand64(R * W, g).view(R, W)
    # layout.encode's array, scattered on the device: the host copy of the
    # encoded database is not needed here.
    enc = torch.zeros((B, 1 << n, W), dtype=torch.int64, device="cuda")
    for j in range(layout.choices):
        enc[torch.from_numpy(layout.candidate_table[:, j]).cuda(),
            torch.from_numpy(layout.position_table[:, j]).cuda()] = db
    rng = np.random.default_rng(3)
    rows = [int(r) for r in rng.choice(R, Q, replace=False)]
    plain, _ = _make_dpf(log_r)
    small, _ = _make_dpf(n)
    p0, p1 = pir.query(plain, rows)
    k0, k1, plan = pir.query_buckets(small, layout, rows)
    d0, d1 = small.upload_key_batch(k0), small.upload_key_batch(k1)
    want = db[torch.tensor(rows, device="cuda")].cpu().numpy().view(np.uint64)
    got = pir.reconstruct_buckets(plan, pir.answer_buckets(small, d0, layout, enc, W),
                                  pir.answer_buckets(small, d1, layout, enc, W), False)
    assert (got == want).all(), "the bucketed protocol returns other records"
    got = pir.reconstruct(pir.answer(plain, p0, db, W), pir.answer(plain, p1, db, W), False)
    assert (got == want).all(), "the plain protocol returns other records"
    out_p = torch.empty((Q, W), dtype=torch.int64, device="cuda")
    out_b = torch.empty((B, W), dtype=torch.int64, device="cuda")
    ms = _timed({"plain": lambda: pir.answer(plain, p0, db, W, out=out_p),
                 "buckets": lambda: pir.answer_buckets(small, d0, layout, enc, W, out=out_b)}, a)
    shape = dict(part="protocol", queries=Q, records=R, record_words=W, buckets=B,
                 log_bucket_size=n, largest_load=int(layout.loads.max()))
    _line("plain", ms["plain"], db_bytes=R * W * 8, **shape)
    _line("buckets", ms["buckets"], db_bytes=B * (1 << n) * W * 8, **shape)
    _ratio("plain_over_buckets", ms["plain"], ms["buckets"], **shape)
    return 0


def part_expand(a):
    import numpy as np
    import torch
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import hip_abi as H
    _setup()
    import oracle as O
    keys = (O.PRG_KEY_LEFT, O.PRG_KEY_RIGHT, O.PRG_KEY_VALUE)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    desc = H.value_desc([(H.LEAF_INT, 64, 0)], True, 2, 1)
    rng = np.random.default_rng(2)

    def dev(x, dtype=np.int64):
        return torch.from_numpy(np.ascontiguousarray(x).view(dtype)).cuda()

    for K, n in ((1 << 16, 12), (1 << 12, 16), (96, 16)):
        dpf, vt = _make_dpf(n)
        alphas = np.zeros((K, 2), dtype=np.uint64)
        alphas[:, 0] = rng.integers(0, 1 << n, size=K, dtype=np.uint64)
        host = dpf.generate_key_batch(alphas, [D.to_value(vt, 7)])[0]
        args = (dev(host.seeds()), dev(host.party(), np.uint8), dev(host.cw_seeds()),
                dev(host.cw_left(), np.uint8), dev(host.cw_right(), np.uint8), keys, desc,
                dev(host.value_correction(0)))
        rows = torch.empty((K, 1 << n), dtype=torch.int64, device="cuda")
        ms = _timed({"expand_rows": lambda: H.expand_rows(n, *args, rows=rows)}, a)
        pl = H.expand_rows_plan(K, n - 1, cus)
        aes = (1 << pl["walk"]) * (pl["walk"] + 2 * ((1 << pl["S"]) - 1) + (1 << pl["S"]))
        ideal = 2 * ((1 << (n - 1)) - 1) + (1 << (n - 1))
        med = float(np.median(ms["expand_rows"]))
        _line("expand_rows", ms["expand_rows"], part="expand", num_keys=K, log_domain_size=n,
              plan=pl, aes_per_key=aes, aes_over_ideal=aes / ideal,
              g_aes_per_s=K * aes / (med * 1e-3) / 1e9,
              row_gbytes_per_s=K * (8 << n) / (med * 1e-3) / 1e9)
        del rows
    return 0


def part_fold(a):
    import numpy as np
    from distributed_point_functions_amd import hip_abi as H
    g = _setup()
    n, W = 16, 32
    N = 1 << n
    desc = H.value_desc([(H.LEAF_INT, 64, 0)], True, 2, 1)
    y = _rand64(B * N, g)
    db = _rand64(B * N * W, g)
    begin = list(range(B + 1))
    import torch
    out = torch.empty((B, W), dtype=torch.int64, device="cuda")
    ws = torch.empty(H.dot_buckets_workspace_bytes(desc, W, B, B, n), dtype=torch.uint8,
                     device="cuda")
    ms = _timed({"dot_buckets": lambda: H.dot_buckets(n, W, begin, desc, y, N * 8, db, out=out,
                                                      workspace=ws)}, a)
    med = float(np.median(ms["dot_buckets"]))
    _line("dot_buckets", ms["dot_buckets"], part="fold", buckets=B, log_bucket_size=n,
          record_words=W, db_bytes=B * N * W * 8, shape=list(H.last_dot_buckets_shape()),
          db_tbytes_per_s=B * N * W * 8 / (med * 1e-3) / 1e12)
    return 0


PARTS = {"gate": part_gate, "protocol": part_protocol, "expand": part_expand, "fold": part_fold}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=list(PARTS), choices=list(PARTS))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per part")
    ap.add_argument("-o", "--output", help="also append the lines to this file")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        return PARTS[a.child](a)
    for part in a.parts:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__),
               "--child", part, "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr)
        if a.output:
            with open(a.output, "a") as f:
                f.write(r.stdout)
        if r.returncode != 0:
            print(f"dot_buckets_ab: part {part} ended with status {r.returncode}; stopping",
                  file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
