"""Additive-share two-server PIR batched over queries.

The protocol: a client that wants record `row` of a database of 2^n records
sends each of the two servers one DPF key for (row, beta).  Each server folds
its full-domain share vector of every key into the database, up to 64 keys
per call and one pass over the records per tile of keys, not per key
(evaluate_dot_batch_to_device).  The two answers add mod 2^64 (XOR for
XorWrapper<uint64>) to beta * db[row] (beta & db[row]): an additive share of
the record, ready for arithmetic MPC.  Single-level DPFs of uint64 or
XorWrapper<uint64>.

The second half is the batch-code form of the same protocol (DESIGN.md section
6j): the database encoded once into buckets by cuckoo hashing (BucketLayout),
one small-domain key per bucket (query_buckets), every key folded into its
own bucket's slice in one call (answer_buckets, reconstruct_buckets).
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


# ---- multi-query PIR over a bucketed database ----------
#
# A batch code by cuckoo hashing: the database of R records is encoded once
# into B buckets, every record lying in `choices` candidate buckets, and a
# client that wants Q <= B records (B about 1.5 Q) places them one per bucket
# and sends one small-domain key per bucket.  A server expands B keys over
# 2^n records each (2^n about choices * R / B) instead of Q keys over R.
# Everything below is a pure function of its arguments, so the two servers
# and the client derive the same layout.

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(x: np.ndarray) -> np.ndarray:
    """splitmix64's finalizer on a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return x ^ (x >> np.uint64(31))


class BucketLayout:
    """Where the records of a database of `num_rows` rows lie in `num_buckets`
    buckets.  The hash: h_j(row) = mix64(mix64(seed + j) ^ row) with mix64
    splitmix64's finalizer; candidate 0 is h_0 mod B, and candidate j is the
    (h_j mod (B - j))-th bucket, in ascending order, among those the earlier
    candidates left, so the `choices` candidates of a row are distinct."""

    def __init__(self, num_rows: int, num_buckets: int, seed: int, choices: int = 3):
        R, B, C = int(num_rows), int(num_buckets), int(choices)
        if R < 1 or C < 1 or B < C:
            raise ValueError("need num_rows >= 1 and num_buckets >= choices >= 1")
        self.num_rows, self.num_buckets, self.seed, self.choices = R, B, int(seed), C
        rows = np.arange(R, dtype=np.uint64)
        cand = np.empty((R, C), dtype=np.int64)
        for j in range(C):
            key = _mix64(np.array([(self.seed + j) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0]
            c = (_mix64(rows ^ key) % np.uint64(B - j)).astype(np.int64)
            taken = np.sort(cand[:, :j], axis=1)
            for i in range(j):
                c += c >= taken[:, i]
            cand[:, j] = c
        self._cand = cand
        # position: the rank of the row among the rows of the bucket, ascending.
        flat_b = cand.reshape(-1)
        order = np.argsort(flat_b, kind="stable")       # row-major: rows ascend within a bucket
        self.loads = np.bincount(flat_b, minlength=B).astype(np.int64)
        first = np.concatenate(([0], np.cumsum(self.loads)[:-1]))
        pos = np.empty(R * C, dtype=np.int64)
        pos[order] = np.arange(R * C, dtype=np.int64) - first[flat_b[order]]
        self._pos = pos.reshape(R, C)
        n = 1
        while (1 << n) < int(self.loads.max()):
            n += 1
        self.log_bucket_size = n

    @property
    def candidate_table(self) -> np.ndarray:
        """candidates(row) of every row: an int64 array (num_rows, choices)."""
        return self._cand

    @property
    def position_table(self) -> np.ndarray:
        """position(row, candidate j of row) of every row: int64 (num_rows, choices)."""
        return self._pos

    def candidates(self, row: int):
        """The `choices` distinct buckets that hold `row`."""
        return [int(b) for b in self._cand[int(row)]]

    def position(self, row: int, bucket: int) -> int:
        """The index of `row` in `bucket`, one of its candidates."""
        j = np.nonzero(self._cand[int(row)] == int(bucket))[0]
        if j.size == 0:
            raise ValueError("bucket %d is no candidate of row %d" % (bucket, row))
        return int(self._pos[int(row), j[0]])

    def encode(self, db) -> np.ndarray:
        """The bucketed database: a (B, 2^n, W) uint64 array holding every
        record of `db` (num_rows x W) at position(row, b) of each of its
        candidates b, zero elsewhere."""
        db = np.ascontiguousarray(db).view(np.uint64).reshape(self.num_rows, -1)
        out = np.zeros((self.num_buckets, 1 << self.log_bucket_size, db.shape[1]), np.uint64)
        for j in range(self.choices):
            out[self._cand[:, j], self._pos[:, j]] = db
        return out

    def schedule(self, rows: Sequence[int], max_evictions: int = 500):
        """A bucket of its own for each of the distinct `rows`, one of its
        candidates (cuckoo insertion: a row finding its candidates taken
        evicts one of their occupants, candidate by candidate in turn, at most
        max_evictions times per insertion).  Returns the buckets in the order
        of `rows`; ValueError when the rows repeat, are more than the buckets
        or find no placement."""
        rows = [int(r) for r in rows]
        if len(set(rows)) != len(rows):
            raise ValueError("the rows of a query must be distinct")
        if any(r < 0 or r >= self.num_rows for r in rows):
            raise ValueError("row out of range")
        if len(rows) > self.num_buckets:
            raise ValueError("more rows than buckets")
        owner = {}        # bucket -> row
        turn = 0
        for r in rows:
            cur = r
            for _ in range(max_evictions + 1):
                cands = self.candidates(cur)
                free = [b for b in cands if b not in owner]
                if free:
                    owner[free[0]] = cur
                    cur = None
                    break
                b = cands[turn % self.choices]
                turn += 1
                cur, owner[b] = owner[b], cur
            if cur is not None:
                raise ValueError("cuckoo insertion failed: no placement found")
        where = {r: b for b, r in owner.items()}
        return [where[r] for r in rows]


class BucketPlan:
    """Which bucket answers which row of a query: buckets[i] serves rows[i]."""

    def __init__(self, rows, buckets, num_buckets):
        self.rows, self.buckets, self.num_buckets = list(rows), list(buckets), int(num_buckets)


def query_buckets(dpf: D.DistributedPointFunction, layout: BucketLayout, rows: Sequence[int],
                  beta=1, root_seeds: Optional[np.ndarray] = None):
    """One key pair per bucket for the distinct records `rows`: the bucket that
    layout.schedule gives a row gets (position of the row, its beta), every
    other bucket (0, 0), so a server cannot tell used buckets from unused
    ones.  `dpf`: single-level, log_domain_size == layout.log_bucket_size.
    `beta`: one integer or one per row; root_seeds: uint64 (2 B, 2) or None
    for fresh randomness.  Returns (host key batch of party 0, of party 1,
    BucketPlan)."""
    p = dpf._parameters[0]
    if len(dpf._parameters) != 1 or p.log_domain_size != layout.log_bucket_size:
        raise ValueError("the DPF must have one level of log_domain_size layout.log_bucket_size")
    betas = [beta] * len(rows) if np.isscalar(beta) else list(beta)
    if len(betas) != len(rows):
        raise ValueError("one beta per row")
    buckets = layout.schedule(rows)
    alphas = [0] * layout.num_buckets
    values = [0] * layout.num_buckets
    for r, b, v in zip(rows, buckets, betas):
        alphas[b] = layout.position(r, b)
        values[b] = int(v)
    k0, k1 = dpf.generate_key_batch_with_betas(
        alphas, [D.to_value(p.value_type, v) for v in values], root_seeds)
    return k0, k1, BucketPlan(rows, buckets, layout.num_buckets)


def answer_buckets(dpf: D.DistributedPointFunction, dev_keys, layout_or_bucket_begin, db_buckets,
                   record_words: int, out=None, stream=None):
    """One server's answers to a device key batch over the bucketed database
    `db_buckets` (torch device tensor, layout.encode's array): a torch int64
    device tensor (K, record_words) of uint64 shares.  A BucketLayout means
    one key per bucket, as query_buckets makes them; else the B + 1 integers
    bucket_begin of evaluate_dot_buckets_to_device (several clients' batches
    merged bucket by bucket)."""
    import torch
    W = int(record_words)
    if isinstance(layout_or_bucket_begin, BucketLayout):
        begin = list(range(layout_or_bucket_begin.num_buckets + 1))
    else:
        begin = [int(x) for x in layout_or_bucket_begin]
    if out is None:
        out = torch.empty((begin[-1], W), dtype=torch.int64, device=db_buckets.device)
    dpf.evaluate_dot_buckets_to_device(dev_keys, 0, begin, db_buckets, W, out, stream=stream)
    return out


def reconstruct_buckets(plan: BucketPlan, a0, a1, xor: bool) -> np.ndarray:
    """The records of plan.rows, in that order, from the two servers' answers
    to a query_buckets batch (one row per bucket each)."""
    both = reconstruct(a0, a1, xor).reshape(plan.num_buckets, -1)
    return both[np.asarray(plan.buckets, dtype=np.int64)]


def _host_u64(x) -> np.ndarray:
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint64)
