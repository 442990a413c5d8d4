#!/usr/bin/env python3
"""Same-box, same-process timing of the database fold ("Database
fold"): HIP events around each launch sequence, a warm-up, then `--reps`
rounds in which the variants alternate; prints one JSON line per variant with
the median and the spread.  Random seeds and correction words: timing only,
parity is the tests' job.

  --levels 29 --words 1   2^30 uint64_t, W = 1:
      (a) expand       dpf_hip_expand into a device buffer
      (b) fused        dpf_hip_expand_dot
      (c) streamed     per slab dpf_hip_expand into scratch + dpf_hip_dot_rows
  --levels 23 --words 32  2^24 records of 32 words:
      (c) streamed, and (d) rows: dpf_hip_dot_rows alone over the whole
      database, beside the time its bytes take at 6.3 TB/s
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12   # achievable HBM rate of the MI355X (float4 copy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=29)
    ap.add_argument("--words", type=int, default=1)
    ap.add_argument("--slab-log", type=int, default=25, help="log2 elements per streamed slab")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch
    from distributed_point_functions_amd import hip_abi as H
    H.load(require_gpu=True)
    dev = torch.device("cuda")
    s = torch.cuda.current_stream()
    g = torch.Generator(device=dev)
    g.manual_seed(7)

    def rand_blocks(n):
        return torch.randint(-2**63, 2**63 - 1, (n, 2), dtype=torch.int64, device=dev, generator=g)

    keys = (0x5be037ccf6a03de5935f08d0a5b6a2fd, 0xef94b6aedebb026ce2ea1fe0f66f4d0b,
            0x05a5d1588c5423e346a31101b21d1c98)
    desc = H.value_desc([(H.LEAF_INT, 64, 0)], True, 2, 1)
    L, W = a.levels, a.words
    n = 2 << L
    slab_levels = min(L, a.slab_log - 1)
    slabs = 1 << (L - slab_levels)
    slab_rows = 2 << slab_levels
    seed, ctrl = rand_blocks(1), torch.zeros(1, dtype=torch.uint8, device=dev)
    slab_seeds = rand_blocks(slabs)
    slab_ctrl = torch.zeros(slabs, dtype=torch.uint8, device=dev)
    cws = rand_blocks(L)
    cl = torch.randint(0, 2, (L,), dtype=torch.uint8, device=dev, generator=g)
    cr = torch.randint(0, 2, (L,), dtype=torch.uint8, device=dev, generator=g)
    vcw = rand_blocks(2)
    db = torch.randint(-2**63, 2**63 - 1, (n * W,), dtype=torch.int64, device=dev, generator=g)
    ws = torch.empty(H.dot_workspace_bytes(desc, W), dtype=torch.uint8, device=dev)
    res = torch.empty(W * 8, dtype=torch.uint8, device=dev)
    scratch = torch.empty(slab_rows * 8, dtype=torch.uint8, device=dev)
    sub = L - slab_levels   # the slabs' expansions use the correction words below the cut

    def streamed():
        for i in range(slabs):
            H.expand(slab_seeds[i:i + 1], slab_ctrl[i:i + 1], cws[sub:], cl[sub:], cr[sub:], keys,
                     desc, 2, vcw, 0, out=scratch)
            H.dot_rows(slab_rows, W, desc, scratch, db[i * slab_rows * W:], accumulate=i > 0,
                       workspace=ws, out=res)

    variants = {"streamed": streamed}
    if W == 1:
        out = torch.empty(n * 8, dtype=torch.uint8, device=dev)
        variants["expand"] = lambda: H.expand(seed, ctrl, cws, cl, cr, keys, desc, 2, vcw, 0, out=out)
        variants["fused"] = lambda: H.expand_dot(seed, ctrl, cws, cl, cr, keys, desc, 2, vcw, 0, db,
                                                 1, workspace=ws, out=res)
    else:
        y = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g)
        variants["rows"] = lambda: H.dot_rows(n, W, desc, y, db, workspace=ws, out=res)

    paths = {}
    for name, fn in variants.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        paths[name] = {"expand": H.last_expand_kernel()[0]}
        if name != "expand":
            paths[name]["dot"] = H.last_dot_kernel()
    ms = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, fn in variants.items():
            e0, e1 = H.Event(), H.Event()
            e0.record(s)
            fn()
            e1.record(s)
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_ms(e1))
    for name, v in ms.items():
        line = {"variant": name, "levels": L, "record_words": W, "records": n, "reps": len(v),
                "ms_median": float(np.median(v)), "ms_min": float(np.min(v)),
                "ms_max": float(np.max(v)), "last_kernels": paths[name]}
        if name == "streamed":
            line["slabs"] = slabs
        if name == "rows":
            line["db_bytes"] = n * W * 8
            line["ms_at_hbm_rate"] = n * W * 8 / HBM_BYTES_PER_S * 1e3
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
