"""Additive-share two-server PIR batched over queries.

The protocol: a client that wants record `row` of a database of 2^n records
sends each of the two servers one DPF key for (row, beta).  Each server folds
its full-domain share vector of every key into the database, up to 64 keys
per call and one pass over the records per tile of keys, not per key
(evaluate_dot_batch_to_device).  The two answers add mod 2^64 (XOR for
XorWrapper<uint64>) to beta * db[row] (beta & db[row]): an additive share of
the record, ready for arithmetic MPC.  Single-level DPFs of uint64 or
XorWrapper<uint64>.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import dpf as D


def query(dpf: D.DistributedPointFunction, rows: Sequence[int], beta=1,
          root_seeds: Optional[Sequence] = None):
    """The two servers' key lists for the records `rows`.  `beta`: one integer
    for every query or one per query; root_seeds: one (seed0, seed1) pair per
    query, or None for fresh randomness."""
    vt = dpf._parameters[0].value_type
    betas = [beta] * len(rows) if np.isscalar(beta) else list(beta)
    if len(betas) != len(rows) or (root_seeds is not None and len(root_seeds) != len(rows)):
        raise ValueError("one beta and one seed pair per row")
    pairs = [dpf.generate_keys_incremental(
        int(r), [D.to_value(vt, int(b))],
        seeds=None if root_seeds is None else (int(root_seeds[i][0]), int(root_seeds[i][1])))
        for i, (r, b) in enumerate(zip(rows, betas))]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def answer(dpf: D.DistributedPointFunction, keys, db, record_words: int, out=None, stream=None):
    """One server's answers to its keys: a torch int64 device tensor of shape
    (len(keys), record_words) holding the uint64 shares.  `db`: torch device
    tensor, 2^n rows of record_words 64-bit words.  More than 64 keys go in
    batches of 64."""
    import torch
    W = int(record_words)
    if out is None:
        out = torch.empty((len(keys), W), dtype=torch.int64, device=db.device)
    flat = out.view(-1)
    for q0 in range(0, len(keys), 64):
        part = keys[q0:q0 + 64]
        dpf.evaluate_dot_batch_to_device(part, 0, db, W, flat[q0 * W:(q0 + len(part)) * W],
                                         stream=stream)
    return out


def reconstruct(a0, a1, xor: bool) -> np.ndarray:
    """The two servers' answers combined: uint64 sums mod 2^64, or XOR."""
    a = _host_u64(a0)
    b = _host_u64(a1)
    return a ^ b if xor else a + b


def _host_u64(x) -> np.ndarray:
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint64)
