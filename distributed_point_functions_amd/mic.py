"""Python mirror of the reference's MultipleIntervalContainmentGate
(dcf/fss_gates/multiple_interval_containment.h:37-87; eprint 2020/1392 Fig. 14),
backed by the host C++ class of csrc/host/multiple_interval_containment.cc whose
evaluation runs in the gfx950 kernels of dpf_hip_mic_eval_batch.  Same names
(snake_case), argument meaning and errors (DpfStatusError with the reference's
messages)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import dpf as D
from . import proto as pb


def make_parameters(log_group_size: int, intervals: Sequence[Tuple[int, int]]) -> pb.MicParameters:
    """MicParameters for the public intervals [(p, q), ...] over Z_{2^log_group_size}."""
    p = pb.MicParameters()
    p.log_group_size = log_group_size
    for lo, hi in intervals:
        iv = p.intervals.add()
        iv.lower_bound.value_uint128.high = int(lo) >> 64
        iv.lower_bound.value_uint128.low = int(lo) & (2**64 - 1)
        iv.upper_bound.value_uint128.high = int(hi) >> 64
        iv.upper_bound.value_uint128.low = int(hi) & (2**64 - 1)
    return p


def _ints(a: np.ndarray) -> List[int]:
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 2)
    return [(int(h) << 64) | int(l) for l, h in a]


class MultipleIntervalContainmentGate:
    """h:37-87.  Construct with create()."""

    def __init__(self, impl, parameters: pb.MicParameters):
        self._impl = impl
        self._parameters = parameters

    @staticmethod
    def create(parameters: pb.MicParameters) -> "MultipleIntervalContainmentGate":
        impl = D._call(D.host().MultipleIntervalContainmentGate.create,
                       parameters.SerializeToString())
        return MultipleIntervalContainmentGate(impl, parameters)

    def parameters(self) -> pb.MicParameters:
        return self._parameters

    def num_intervals(self) -> int:
        return len(self._parameters.intervals)

    def num_unique_offsets(self) -> int:
        """DCF evaluations per gate: distinct p_i and q_i + 1 (at most 2 m)."""
        return self._impl.num_unique_offsets()

    def gen(self, r_in: int, r_out: Sequence[int], seed_0: Optional[int] = None,
            seed_1: Optional[int] = None, z_0: Optional[Sequence[int]] = None):
        """Fig. 14 Gen (cc:104-204).  With seed_0, seed_1 (the DCF's root seeds)
        and z_0 (party 0's mask shares, one per interval) the keys are
        reproducible; all three or none."""
        given = [seed_0 is not None, seed_1 is not None, z_0 is not None]
        if any(given) and not all(given):
            raise ValueError("seed_0, seed_1 and z_0 go together")
        ro = D.u128_array(list(r_out))
        if all(given):
            k0, k1 = D._call(self._impl.gen, int(r_in), ro, int(seed_0), int(seed_1),
                             D.u128_array(list(z_0)))
        else:
            k0, k1 = D._call(self._impl.gen, int(r_in), ro)
        a, b = pb.MicKey(), pb.MicKey()
        a.ParseFromString(k0)
        b.ParseFromString(k1)
        return a, b

    def eval(self, key: pb.MicKey, x: int) -> List[int]:
        """Fig. 14 Eval (cc:206-275): one share in Z_N per interval."""
        return _ints(D._call(self._impl.eval, key.SerializeToString(), int(x)))

    def eval_batch(self, keys: Sequence[pb.MicKey], xs: Sequence[int]) -> List[List[int]]:
        """eval(keys[g], xs[g]) for every g, in one launch."""
        m = self.num_intervals()
        flat = _ints(D._call(self._impl.eval_batch, [k.SerializeToString() for k in keys],
                             D.u128_array(list(xs))))
        return [flat[g * m:(g + 1) * m] for g in range(len(keys))]

    def make_key_batch(self, keys: Sequence[pb.MicKey]):
        return D._call(self._impl.make_key_batch, [k.SerializeToString() for k in keys])

    def _gen_batch_args(self, r_in, r_out, root_seeds, z_0):
        flat = [int(v) for row in r_out for v in row]
        z = None if z_0 is None else D.u128_array([int(v) for row in z_0 for v in row])
        return D.u128_array(list(r_in)), D.u128_array(flat), root_seeds, z

    def gen_batch(self, r_in: Sequence[int], r_out: Sequence[Sequence[int]],
                  root_seeds: Optional[np.ndarray] = None,
                  z_0: Optional[Sequence[Sequence[int]]] = None):
        """gen for many gates at once, straight into key batches: gate g takes
        r_in[g], r_out[g], root_seeds[2g], root_seeds[2g+1] (uint64 (2n, 2)) and
        z_0[g]; None draws fresh randomness.  Returns both parties' batches."""
        return D._call(self._impl.gen_batch, *self._gen_batch_args(r_in, r_out, root_seeds, z_0))

    def gen_batch_to_device(self, r_in: Sequence[int], r_out: Sequence[Sequence[int]],
                            root_seeds: Optional[np.ndarray] = None,
                            z_0: Optional[Sequence[Sequence[int]]] = None, stream=None):
        """The same batches generated in device memory on `stream`."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return D._call(self._impl.gen_batch_to_device,
                       *self._gen_batch_args(r_in, r_out, root_seeds, z_0), s.cuda_stream)

    def download_key_batch(self, device_batch, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return D._call(device_batch.download, s.cuda_stream)

    def upload_key_batch(self, batch, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return D._call(batch.upload, s.cuda_stream)

    def eval_batch_to_device(self, device_batch, xs, out, stream=None) -> int:
        """Eval for every key of a device batch at its masked input xs[key]
        (torch int64 (gates, 2) {low, high}); `out` receives [gate][interval]
        16-byte little-endian values.  Returns the number of values."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        return D._call(self._impl.eval_batch_to_device, device_batch, xs.data_ptr(),
                       out.data_ptr(), out.numel() * out.element_size(), s.cuda_stream)
