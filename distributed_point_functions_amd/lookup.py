"""Private table lookup from DPF key batches.

The protocol: a dealer gives the two parties a DPF key for a random mask r_k
per lookup.  Online the parties open s_k = x_k - r_k mod 2^n, and each folds
its full-domain share vector into the public table rotated by s_k.  The two
results add (XOR for XorWrapper) to beta_k * T[x_k].  The dealer's side is
generate_key_batch_to_device; the parties' side is one fused launch per batch,
evaluate_lookup_batch_to_device, which stores no share vector.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import dpf as D


def deal(dpf: D.DistributedPointFunction, masks: Sequence[int], betas: Sequence,
         root_seeds: Optional[np.ndarray] = None, stream=None):
    """Both parties' device key batches for the masks r_k (the DPFs' alphas).
    `betas`: one value per hierarchy level shared by all keys, or len(masks)
    times that many, key-major.  root_seeds: uint64 (2K, 2) or None for fresh
    randomness."""
    return dpf.generate_key_batch_to_device(masks, betas, root_seeds, stream=stream)


def offsets_for(xs: Sequence[int], masks: Sequence[int], log_domain_size: int) -> np.ndarray:
    """The opened offsets s_k = x_k - r_k mod 2^n as uint64."""
    m = (1 << log_domain_size) - 1
    return np.array([(int(x) - int(r)) & m for x, r in zip(xs, masks)], dtype=np.uint64)


def evaluate(dpf: D.DistributedPointFunction, device_batch, offsets, table, table_words: int,
             hierarchy_level: int = 0, out=None, stream=None):
    """One party's shares of T[(alpha_k + s_k) mod 2^n] for every key of its
    batch: a torch int64 device tensor of shape (K, table_words) holding the
    uint64 sums.  `offsets`: a torch device tensor of K 64-bit words or a host
    sequence; `table`: torch device tensor, 2^n rows of table_words 64-bit
    words."""
    import torch
    K = int(device_batch.num_keys)
    if not isinstance(offsets, torch.Tensor):
        host = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64)).view(np.int64)
        offsets = torch.from_numpy(host).to(table.device)
    if out is None:
        out = torch.empty((K, int(table_words)), dtype=torch.int64, device=table.device)
    dpf.evaluate_lookup_batch_to_device(device_batch, hierarchy_level, offsets, table, table_words,
                                        out, stream=stream)
    return out


def reconstruct(share0, share1, xor: bool) -> np.ndarray:
    """The two parties' shares combined: uint64 sums mod 2^64, or XOR."""
    a = _host_u64(share0)
    b = _host_u64(share1)
    return a ^ b if xor else a + b


def _host_u64(x) -> np.ndarray:
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint64)
