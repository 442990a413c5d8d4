"""Private histograms from DPF key batches.

The protocol: each of K clients splits the unit vector beta_k * e_{alpha_k}
over one flat domain of 2^n bins into a DPF key pair and sends one key to each
of two servers.  A server sums its keys' full-domain evaluations element by
element; the two servers' vectors add (XOR for XorWrapper) to the histogram
sum_k beta_k * e_{alpha_k}.  The clients' side is generate_key_batch_to_device;
a server's side is one fused launch per batch,
evaluate_full_domain_sum_to_device, which stores no share vector and can
stream batch after batch into one accumulator.

Over a field (IntModN<uint32, N>, or the heavy-hitters 2-tuple) the servers can
check every client before counting it: fold_checked gives the field sum and, in
the same launch, each client's linear sketches, which `check` tests for a unit
vector; reconstruct_mod adds the two servers' sums mod N.

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
    accumulating.  A level of 8-, 16- or 32-bit integers (plain or XorWrapper)
    or of XorWrapper<uint128> gives its packed elements: torch uint8, int16 or
    int32 [2^n], or int64 [2^n, 2] (evaluate_full_domain_sum_packed_to_device)."""
    import torch
    n = int(dpf.parameters()[hierarchy_level].log_domain_size)
    if (not dpf.evaluates_full_domain_sum_on_device(hierarchy_level)
            and dpf.evaluates_full_domain_sum_packed_on_device(hierarchy_level)):
        if out is None:
            shape, dtype = {1: ((1 << n,), torch.uint8), 2: ((1 << n,), torch.int16),
                            4: ((1 << n,), torch.int32),
                            16: ((1 << n, 2), torch.int64)}[dpf.packed_size(hierarchy_level)]
            make = torch.zeros if accumulate else torch.empty
            out = make(shape, dtype=dtype, device="cuda")
        dpf.evaluate_full_domain_sum_packed_to_device(device_batch, hierarchy_level, out,
                                                      accumulate=accumulate, stream=stream)
        return out
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


def reconstruct_packed(share0, share1, bits: int, xor: bool) -> np.ndarray:
    """The two servers' packed shares combined element by element: sums mod
    2^bits, or XOR.  uint8, uint16, uint32 or uint64 [N]; uint64 [N, 2] (low
    word first) for 128 bits, which only XOR takes."""
    if bits not in (8, 16, 32, 64, 128) or (bits == 128 and not xor):
        raise ValueError("bits must be 8, 16, 32 or 64, or 128 with xor")
    dtype = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64, 128: np.uint64}[bits]
    a = _host_bits(share0, dtype)
    b = _host_bits(share1, dtype)
    r = a ^ b if xor else a + b
    return r.reshape(-1, 2) if bits == 128 else r.reshape(-1)


def fold_checked(dpf: D.DistributedPointFunction, device_batch, weights, hierarchy_level: int = 0,
                 out=None, accumulate: bool = False, stream=None):
    """One server's share of a checked histogram over a field (DESIGN.md
    section 6h): (sum, sketches), the torch int32 device tensors [2^n, nl] of
    its batch's sums mod N_e and [K, J, nl] of every client's sketches under
    `weights` (uint32 (J, 2^n), J <= 2: heavy_hitters.sketch_weights; None for
    the plain field sum, J = 0), from one launch.  `out`: the sum tensor to
    write (or, with `accumulate`, to add into mod N_e); None makes a fresh one,
    zeroed when accumulating.  The sketches are per batch: always fresh."""
    import torch
    n = int(dpf.parameters()[hierarchy_level].log_domain_size)
    nl = dpf.packed_size(hierarchy_level) // 4
    w = None
    if weights is not None:
        w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.uint32).view(np.int32))
        w = w.reshape(-1, 1 << n).to("cuda")
    J = 0 if w is None else int(w.shape[0])
    if out is None:
        make = torch.zeros if accumulate else torch.empty
        out = make((1 << n, nl), dtype=torch.int32, device="cuda")
    sketches = torch.empty((device_batch.num_keys, J, nl), dtype=torch.int32, device="cuda")
    dpf.evaluate_full_domain_sum_sketch_to_device(hierarchy_level, device_batch, w, out,
                                                  sketches if J else None,
                                                  accumulate=accumulate, stream=stream)
    return out, sketches


def check(s0, s1) -> np.ndarray:
    """bool[K]: which clients' vectors pass the unit-vector test, from the two
    servers' sketches under heavy_hitters.sketch_weights of the heavy-hitters
    value type (heavy_hitters.check_sketches: Z is opened in one process, which
    stands in for the servers' multiplication protocol)."""
    from . import heavy_hitters as HH
    return HH.check_sketches(_host_u32(s0), _host_u32(s1))


def reconstruct_mod(share0, share1, moduli: Sequence[int]) -> np.ndarray:
    """The two servers' field shares combined: uint32 [..., nl], element e
    added mod moduli[e]."""
    m = np.asarray(moduli, dtype=np.uint64)
    a = _host_u32(share0).astype(np.uint64).reshape(-1, len(m))
    b = _host_u32(share1).astype(np.uint64).reshape(-1, len(m))
    return ((a + b) % m).astype(np.uint32)


def _host_u32(x) -> np.ndarray:
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint32)


def _host_bits(x, dtype) -> np.ndarray:
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(dtype)


def _host_u64(x) -> np.ndarray:
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint64)
