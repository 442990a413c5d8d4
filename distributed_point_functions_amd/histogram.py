"""Private histograms from DPF key batches.

The protocol: each of K clients splits the unit vector beta_k * e_{alpha_k}
over one flat domain of 2^n bins into a DPF key pair and sends one key to each
of two servers.  A server sums its keys' full-domain evaluations element by
element; the two servers' vectors add (XOR for XorWrapper) to the histogram
sum_k beta_k * e_{alpha_k}.  The clients' side is generate_key_batch_to_device;
a server's side is one fused launch per batch,
evaluate_full_domain_sum_to_device, which stores no share vector and can
stream batch after batch into one accumulator.

Where the clients of one server are spread over several ranks, each rank folds
its own clients into a vector of its own, and those per-rank vectors are what
sharding.aggregate_shares reduces across the ranks: nothing here adds a
collective.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import dpf as D


def submit(dpf: D.DistributedPointFunction, alphas: Sequence[int], betas: Sequence,
           root_seeds: Optional[np.ndarray] = None, stream=None):
    """Both servers' device key batches for the clients' bins `alphas`.
    `betas`: one value per hierarchy level shared by all keys, or len(alphas)
    times that many, key-major.  root_seeds: uint64 (2K, 2) or None for fresh
    randomness."""
    return dpf.generate_key_batch_to_device(alphas, betas, root_seeds, stream=stream)


def fold(dpf: D.DistributedPointFunction, device_batch, hierarchy_level: int = 0, out=None,
         accumulate: bool = False, stream=None):
    """One server's share of the histogram of its batch: a torch int64 device
    tensor of 2^n words holding the uint64 sums.  `out`: the tensor to write
    (or, with `accumulate`, to add into); None makes a fresh one, zeroed when
    accumulating."""
    import torch
    n = int(dpf.parameters()[hierarchy_level].log_domain_size)
    if out is None:
        make = torch.zeros if accumulate else torch.empty
        out = make(1 << n, dtype=torch.int64, device="cuda")
    dpf.evaluate_full_domain_sum_to_device(device_batch, hierarchy_level, out,
                                           accumulate=accumulate, stream=stream)
    return out


def reconstruct(share0, share1, xor: bool) -> np.ndarray:
    """The two servers' shares combined: uint64 sums mod 2^64, or XOR."""
    a = _host_u64(share0)
    b = _host_u64(share1)
    return a ^ b if xor else a + b


def _host_u64(x) -> np.ndarray:
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint64)
