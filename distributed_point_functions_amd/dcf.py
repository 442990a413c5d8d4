"""Python mirror of the reference's DistributedComparisonFunction
(dcf/distributed_comparison_function.h:30-105), backed by the host C++ class
of csrc/host/distributed_comparison_function.cc whose evaluation runs in the
gfx950 kernel dpf_hip_dcf_eval_batch (point by point) or dpf_hip_dcf_expand
(the whole domain).  Same names (snake_case), argument
meaning and errors (DpfStatusError with the reference's messages)."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import dpf as D
from . import proto as pb


class DistributedComparisonFunction:
    """h:30-74.  Construct with create()."""

    def __init__(self, impl, parameters: pb.DcfParameters):
        self._impl = impl
        self._parameters = parameters

    @staticmethod
    def create(parameters: pb.DcfParameters) -> "DistributedComparisonFunction":
        impl = D._call(D.host().DistributedComparisonFunction.create,
                       parameters.SerializeToString())
        return DistributedComparisonFunction(impl, parameters)

    def parameters(self) -> pb.DcfParameters:
        return self._parameters

    def value_type(self) -> pb.ValueType:
        return self._parameters.parameters.value_type

    def generate_keys(self, alpha: int, beta, seed_0: Optional[int] = None,
                      seed_1: Optional[int] = None):
        """Keys for x -> beta if x < alpha else 0 (cc:79-101).  `beta` is a Value
        proto or a Python value of the DCF's value type; seeds (optional) make
        the keys reproducible."""
        if not isinstance(beta, pb.Value):
            beta = D.to_value(self.value_type(), beta)
        k0, k1 = D._call(self._impl.generate_keys, int(alpha), beta.SerializeToString(),
                         None if seed_0 is None else int(seed_0),
                         None if seed_1 is None else int(seed_1))
        a, b = pb.DcfKey(), pb.DcfKey()
        a.ParseFromString(k0)
        b.ParseFromString(k1)
        return a, b

    def evaluate_packed(self, key: pb.DcfKey, xs: Sequence[int],
                        value_type: Optional[pb.ValueType] = None) -> np.ndarray:
        pts = xs if isinstance(xs, np.ndarray) else D.u128_array(xs)
        out = D._call(self._impl.evaluate, key.SerializeToString(), pts,
                      None if value_type is None else value_type.SerializeToString())
        size = self._impl.packed_size()
        return out.reshape(-1, size)

    def evaluate(self, key: pb.DcfKey, x: int, value_type: Optional[pb.ValueType] = None):
        """h:83-105: the share of [x < alpha] * beta (Python int or tuple)."""
        vt = value_type if value_type is not None else self.value_type()
        return D.decode(vt, self.evaluate_packed(key, [x], value_type))[0]

    def make_key_batch(self, keys: Sequence[pb.DcfKey]):
        return D._call(self._impl.make_key_batch, [k.SerializeToString() for k in keys])

    def _betas(self, betas):
        vt = self.value_type()
        return [(b if isinstance(b, pb.Value) else D.to_value(vt, b)).SerializeToString()
                for b in betas]

    def generate_key_batch(self, alphas: Sequence[int], betas: Sequence,
                           root_seeds: Optional[np.ndarray] = None, threads: int = 0):
        """Both parties' key batches for every alpha, on host threads: row k is
        generate_keys(alphas[k], beta_k, seeds) through make_key_batch.  `betas`
        holds one value for all keys or one per key; root_seeds: uint64 (2n, 2)
        or None for fresh randomness."""
        al = alphas if isinstance(alphas, np.ndarray) else D.u128_array(alphas)
        return D._call(self._impl.generate_key_batch, al, self._betas(betas), root_seeds,
                       int(threads))

    def generate_key_batch_to_device(self, alphas: Sequence[int], betas: Sequence,
                                     root_seeds: Optional[np.ndarray] = None, stream=None):
        """The same batches generated in device memory on `stream`."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        al = alphas if isinstance(alphas, np.ndarray) else D.u128_array(alphas)
        return D._call(self._impl.generate_key_batch_to_device, al, self._betas(betas),
                       root_seeds, s.cuda_stream)

    def generates_keys_on_device(self) -> bool:
        return self._impl.generates_keys_on_device()

    def download_key_batch(self, device_batch, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return D._call(device_batch.download, s.cuda_stream)

    def upload_key_batch(self, batch, begin: int = 0, end: Optional[int] = None, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        end = batch.num_keys if end is None else end
        return D._call(batch.upload, int(begin), int(end), s.cuda_stream)

    def evaluate_batch_to_device(self, device_batch, points, points_per_key: int, out,
                                 shared_points: bool = False, stream=None) -> int:
        """Evaluate for every key of a device batch at device points (torch int64
        (n, 2) {low, high}); packed [key][point] outputs in `out`."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        return D._call(self._impl.evaluate_batch_to_device, device_batch, points.data_ptr(),
                       int(points_per_key), bool(shared_points), out.data_ptr(),
                       out.numel() * out.element_size(), s.cuda_stream)

    # ---- full-domain evaluation (one depth-first walk of the key's tree) ----
    def evaluates_full_domain_on_device(self) -> bool:
        """True for the value types the full-domain kernel takes (one integer or
        XorWrapper of 8 to 128 bits); the calls below are UNIMPLEMENTED for
        every other type -- no per-point path stands in for them."""
        return self._impl.evaluates_full_domain_on_device()

    def evaluate_full_domain_to_device(self, key: pb.DcfKey, out, shard: int = 0,
                                       num_shards: int = 1, stream=None) -> int:
        """The shares of evaluate(key, x) at every x of shard `shard` of
        `num_shards` (a power of two; the x whose top bits are `shard`), packed
        [x - first_x] into the device tensor `out`; returns the element count."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        return D._call(self._impl.evaluate_full_domain_to_device, key.SerializeToString(),
                       int(shard), int(num_shards), out.data_ptr(),
                       out.numel() * out.element_size(), s.cuda_stream)

    def evaluate_full_domain_batch_to_device(self, device_batch, out, shard: int = 0,
                                             num_shards: int = 1, stream=None) -> int:
        """The same for every key of a device batch: packed [key][x - first_x]."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        return D._call(self._impl.evaluate_full_domain_batch_to_device, device_batch, int(shard),
                       int(num_shards), out.data_ptr(), out.numel() * out.element_size(),
                       s.cuda_stream)

    def evaluate_full_domain_packed(self, key: pb.DcfKey,
                                    value_type: Optional[pb.ValueType] = None) -> np.ndarray:
        """The whole domain on the host: uint8 (2^n, packed_size)."""
        out = D._call(self._impl.evaluate_full_domain_packed, key.SerializeToString(),
                      None if value_type is None else value_type.SerializeToString())
        return out.reshape(-1, self._impl.packed_size())

    def evaluate_range_dot_to_device(self, key: pb.DcfKey, db, record_words: int, out,
                                     shard: int = 0, num_shards: int = 1, stream=None) -> int:
        """Private range query (uint64 DCFs): out[w] = sum over the shard's x of
        f(x) * db[x - first_x][w] mod 2^64; the two parties' results add to
        beta * sum(db[x][w] for x < alpha).  `db` is the shard's records as a
        device tensor of record_words uint64 each."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        return D._call(self._impl.evaluate_range_dot_to_device, key.SerializeToString(),
                       int(shard), int(num_shards), db.data_ptr(),
                       db.numel() * db.element_size(), int(record_words), out.data_ptr(),
                       out.numel() * out.element_size(), s.cuda_stream)

    def evaluate_range_dot(self, key: pb.DcfKey, db, record_words: int) -> np.ndarray:
        """The whole domain's fold on the host: uint64 (record_words,)."""
        return D._call(self._impl.evaluate_range_dot, key.SerializeToString(), db.data_ptr(),
                       db.numel() * db.element_size(), int(record_words))

    def packed_size(self) -> int:
        return self._impl.packed_size()
