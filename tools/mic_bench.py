"""A/B of the batched multiple-interval-containment gate against the DCF route
to the same DCF values.

One process, alternating per repeat, device events around each call:
  (a) MultipleIntervalContainmentGate.eval_batch_to_device: one masked input
      per gate; the walks over the |U| distinct offsets plus the combine.
  (b) DistributedComparisonFunction.evaluate_batch_to_device on the |U|
      precomputed device points per key -- that call alone (no combine).
  (c) the same on the undeduplicated 2 m points per key: what the offset
      deduplication buys.
The bar: median(a) <= median(b) + (max(b) - min(b)).

Usage (GPU box, repo root): python tools/mic_bench.py [--log-gates 16]
    [--intervals 8] [--log-group 64] [--repeats 12] [--distinct-keys 4096]
Prints walks, AES blocks (gates * |U| * (2n - 1)), and per leg ms and G AES/s.
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def u128_rows(values):
    a = np.empty((len(values), 2), np.uint64)
    a[:, 0] = [v & (2**64 - 1) for v in values]
    a[:, 1] = [v >> 64 for v in values]
    return a


def main():
    import torch
    from distributed_point_functions_amd import dcf as C
    from distributed_point_functions_amd import mic as M
    from distributed_point_functions_amd import proto as pb
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-gates", type=int, default=16)
    ap.add_argument("--intervals", type=int, default=8)
    ap.add_argument("--log-group", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--distinct-keys", type=int, default=4096,
                    help="key pairs generated; the batch cycles through them")
    a = ap.parse_args()
    n, m, gates = a.log_group, a.intervals, 1 << a.log_gates
    N = 1 << n
    cuts = [i * N // m for i in range(m)] + [N]
    intervals = [(cuts[i], cuts[i + 1] - 1) for i in range(m)]      # a partition of Z_N
    g = M.MultipleIntervalContainmentGate.create(M.make_parameters(n, intervals))
    nu = g.num_unique_offsets()
    rng = np.random.default_rng(1)
    big = lambda: int.from_bytes(rng.bytes(16), "little") % N        # noqa: E731
    distinct = min(a.distinct_keys, gates)
    pool = [g.gen(big(), [big() for _ in range(m)])[i % 2] for i in range(distinct)]
    keys = [pool[i % distinct] for i in range(gates)]
    xs = [big() for _ in range(gates)]
    dev = g.upload_key_batch(g.make_key_batch(keys))
    dx = torch.from_numpy(u128_rows(xs).view(np.int64)).cuda()
    out_a = torch.empty(gates * m * 16, dtype=torch.uint8, device="cuda")

    p = pb.DcfParameters()
    p.parameters.log_domain_size = n
    p.parameters.value_type.integer.bitsize = 128
    dcf = C.DistributedComparisonFunction.create(p)
    ddev = dcf.upload_key_batch(dcf.make_key_batch([k.dcfkey for k in keys]))
    lower = [lo for lo, _ in intervals]
    upper_next = [(hi + 1) % N for _, hi in intervals]
    offsets = sorted(set(lower) | set(upper_next))
    assert len(offsets) == nu

    def points(offs):
        return torch.from_numpy(
            u128_rows([(x + N - 1 - o) % N for x in xs for o in offs]).view(np.int64)).cuda()

    pts_b, pts_c = points(offsets), points(lower + upper_next)
    out_b = torch.empty(gates * nu * 16, dtype=torch.uint8, device="cuda")
    out_c = torch.empty(gates * 2 * m * 16, dtype=torch.uint8, device="cuda")
    legs = [
        ("a mic.eval_batch_to_device", nu, lambda: g.eval_batch_to_device(dev, dx, out_a)),
        ("b dcf |U| points", nu, lambda: dcf.evaluate_batch_to_device(ddev, pts_b, nu, out_b)),
        ("c dcf 2m points", 2 * m, lambda: dcf.evaluate_batch_to_device(ddev, pts_c, 2 * m, out_c)),
    ]
    aes_per_walk = 2 * n - 1
    print(f"gates {gates} intervals {m} log_group {n} |U| {nu}: walks {gates * nu}, "
          f"AES blocks {gates * nu * aes_per_walk} (undeduplicated {gates * 2 * m * aes_per_walk})",
          flush=True)
    for _, _, fn in legs:      # warm: buffers, tables, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in legs}
    for r in range(a.repeats):
        for name, ppk, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1)
            ms[name].append(t)
            print(f"repeat {r} {name}: {t:.4f} ms {gates * ppk * aes_per_walk / t / 1e6:.1f} G AES/s",
                  flush=True)
    med = {}
    for name, ppk, _ in legs:
        v = ms[name]
        med[name] = statistics.median(v)
        print(f"median {name}: {med[name]:.4f} ms (min {min(v):.4f} max {max(v):.4f}) "
              f"{gates * ppk * aes_per_walk / med[name] / 1e6:.1f} G AES/s", flush=True)
    (na, _, _), (nb, _, _), (nc, _, _) = legs
    spread = max(ms[nb]) - min(ms[nb])
    print(f"bar: median(a) {med[na]:.4f} <= median(b) {med[nb]:.4f} + spread(b) {spread:.4f} = "
          f"{med[nb] + spread:.4f} ms: {'met' if med[na] <= med[nb] + spread else 'MISSED'}")
    print(f"deduplication: median(c) / median(a) = {med[nc] / med[na]:.3f}")
    try:
        print(f"shader clock after the run: {torch.cuda.clock_rate()} MHz")
    except Exception as e:   # the management library may be absent
        print(f"shader clock: unavailable ({type(e).__name__})")


if __name__ == "__main__":
    main()
