"""Python mirror of the reference's DistributedPointFunction API
(dpf/distributed_point_function.h:77-365), backed by the host C++ library
(lib/libdpf.so via the _dpf_host pybind module), whose evaluation runs in the
gfx950 kernels of lib/libdpf_hip.so.  Same method names (snake_case), argument
meaning and error behaviour: failing calls raise DpfStatusError carrying the
absl status code and the reference's message.

Outputs: evaluate_* return numpy arrays.  For single-leaf types of <= 64 bits
the array has the natural dtype (uint8/16/32/64); otherwise it is the packed
element layout, shape (n, packed_size) uint8 (leaves concatenated
little-endian); decode() turns either into Python values.
"""
from __future__ import annotations

import os
import sys
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import proto as pb

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBDIR = os.path.join(_HERE, "lib")
_host = None

STATUS_NAMES = {0: "OK", 3: "INVALID_ARGUMENT", 8: "RESOURCE_EXHAUSTED", 9: "FAILED_PRECONDITION",
                12: "UNIMPLEMENTED", 13: "INTERNAL", 11: "OUT_OF_RANGE", 5: "NOT_FOUND"}
MASK64 = (1 << 64) - 1


class DpfStatusError(Exception):
    def __init__(self, code: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {message}")
        self.code = code
        self.code_name = STATUS_NAMES.get(code, str(code))
        self.message = message


def host():
    """Loads the pybind module (after torch, so one HIP runtime is shared)."""
    global _host
    if _host is None:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if _LIBDIR not in sys.path:
            sys.path.insert(0, _LIBDIR)
        try:
            import _dpf_host  # noqa: F401
        except ImportError as e:
            raise DpfStatusError(13, f"host library not built ({e}); run "
                                     "python -m distributed_point_functions_amd.build_native")
        _host = _dpf_host
    return _host


def _call(fn, *args):
    try:
        return fn(*args)
    except host().StatusError as e:
        code, _, msg = str(e).partition("|")
        raise DpfStatusError(int(code), msg) from None


def u128_from_block(b) -> int:
    """Python int of a proto Block {high, low}."""
    return (int(b.high) << 64) | int(b.low)


def u128_array(xs: Sequence[int]) -> np.ndarray:
    a = np.empty((len(xs), 2), dtype=np.uint64)
    for i, x in enumerate(xs):
        x = int(x)
        a[i, 0] = x & MASK64
        a[i, 1] = (x >> 64) & MASK64
    return a


# ---------------------------------------------------------------- value types
def integer_type(bits: int) -> pb.ValueType:
    vt = pb.ValueType()
    vt.integer.bitsize = bits
    return vt


def xor_wrapper_type(bits: int) -> pb.ValueType:
    vt = pb.ValueType()
    vt.xor_wrapper.bitsize = bits
    return vt


def int_mod_n_type(base_bits: int, modulus: int) -> pb.ValueType:
    vt = pb.ValueType()
    vt.int_mod_n.base_integer.bitsize = base_bits
    _set_integer(vt.int_mod_n.modulus, modulus)
    return vt


def tuple_type(*elements: pb.ValueType) -> pb.ValueType:
    vt = pb.ValueType()
    vt.tuple.SetInParent()
    for e in elements:
        vt.tuple.elements.add().CopyFrom(e)
    return vt


def _set_integer(msg, v: int):
    # Uint128ToValueInteger (value_type_helpers.cc:134-144)
    v = int(v)
    if v >> 64 == 0:
        msg.value_uint64 = v
    else:
        msg.value_uint128.high = v >> 64
        msg.value_uint128.low = v & MASK64


def _get_integer(msg) -> int:
    which = msg.WhichOneof("value")
    if which == "value_uint128":
        return (msg.value_uint128.high << 64) | msg.value_uint128.low
    return msg.value_uint64


def to_value(vt: pb.ValueType, x) -> pb.Value:
    """ToValue for a runtime ValueType: ints for leaves, sequences for tuples."""
    v = pb.Value()
    kind = vt.WhichOneof("type")
    if kind == "integer":
        _set_integer(v.integer, x)
    elif kind == "int_mod_n":
        _set_integer(v.int_mod_n, x)
    elif kind == "xor_wrapper":
        _set_integer(v.xor_wrapper, x)
    elif kind == "tuple":
        v.tuple.SetInParent()
        for et, ex in zip(vt.tuple.elements, x):
            v.tuple.elements.add().CopyFrom(to_value(et, ex))
    else:
        raise ValueError("unsupported value type")
    return v


def from_value(vt: pb.ValueType, v: pb.Value):
    kind = vt.WhichOneof("type")
    if kind == "tuple":
        return tuple(from_value(et, ev) for et, ev in zip(vt.tuple.elements, v.tuple.elements))
    return _get_integer(getattr(v, kind))


def leaves_of(vt: pb.ValueType) -> List[Tuple[str, int, int]]:
    kind = vt.WhichOneof("type")
    if kind == "integer":
        return [("int", vt.integer.bitsize, 0)]
    if kind == "xor_wrapper":
        return [("xor", vt.xor_wrapper.bitsize, 0)]
    if kind == "int_mod_n":
        return [("intmodn", vt.int_mod_n.base_integer.bitsize, _get_integer(vt.int_mod_n.modulus))]
    out = []
    for e in vt.tuple.elements:
        out += leaves_of(e)
    return out


def decode(vt: pb.ValueType, arr: np.ndarray) -> list:
    """Packed or natural-dtype output -> list of Python values (nested tuples)."""
    ls = leaves_of(vt)
    size = sum(b // 8 for _, b, _ in ls)
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1, size)
    out = []
    for row in raw:
        b = row.tobytes()
        vals, off = [], 0
        for _, bits, _ in ls:
            vals.append(int.from_bytes(b[off:off + bits // 8], "little"))
            off += bits // 8
        it = iter(vals)
        out.append(_rebuild(vt, it))
    return out


def _rebuild(vt, it):
    if vt.WhichOneof("type") == "tuple":
        return tuple(_rebuild(e, it) for e in vt.tuple.elements)
    return next(it)


def _natural(vt: pb.ValueType, packed: np.ndarray, n: int) -> np.ndarray:
    ls = leaves_of(vt)
    size = sum(b // 8 for _, b, _ in ls)
    packed = packed.reshape(n, size) if n else packed.reshape(0, size)
    if len(ls) == 1 and ls[0][1] <= 64:
        return packed.view({8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}[ls[0][1]]).reshape(-1)
    return packed


class DistributedPointFunction:
    """h:77-365.  Construct with create() / create_incremental()."""

    def __init__(self, impl, parameters: List[pb.DpfParameters]):
        self._impl = impl
        self._parameters = parameters

    @staticmethod
    def create(parameters: pb.DpfParameters) -> "DistributedPointFunction":
        return DistributedPointFunction.create_incremental([parameters])

    @staticmethod
    def create_incremental(parameters: Sequence[pb.DpfParameters]) -> "DistributedPointFunction":
        impl = _call(host().DistributedPointFunction.create_incremental,
                     [p.SerializeToString() for p in parameters])
        params = []
        for b in impl.parameters():
            p = pb.DpfParameters()
            p.ParseFromString(b)
            params.append(p)
        return DistributedPointFunction(impl, params)

    def parameters(self) -> List[pb.DpfParameters]:
        return list(self._parameters)

    def register_value_type(self, value_type: pb.ValueType) -> None:
        _call(self._impl.register_value_type, value_type.SerializeToString())

    def to_value(self, value_type: pb.ValueType, x) -> pb.Value:
        self.register_value_type(value_type)
        return to_value(value_type, x)

    # -- key generation (CPU) ------------------------------------------------
    def _betas(self, beta) -> List[bytes]:
        out = []
        for b in beta:
            if isinstance(b, pb.Value):
                out.append(b.SerializeToString())
            else:  # plain integer (uint128 overload, h:160-164)
                out.append(to_value(integer_type(128), b).SerializeToString())
        return out

    def generate_keys(self, alpha: int, beta) -> Tuple[pb.DpfKey, pb.DpfKey]:
        return self.generate_keys_incremental(alpha, [beta])

    def generate_keys_incremental(self, alpha: int, beta: Sequence,
                                  seeds: Optional[Tuple[int, int]] = None):
        if seeds is None:
            a, b = _call(self._impl.generate_keys_incremental, int(alpha), self._betas(beta))
        else:
            a, b = _call(self._impl.generate_keys_incremental_with_seeds, int(alpha),
                         self._betas(beta), int(seeds[0]), int(seeds[1]))
        k0, k1 = pb.DpfKey(), pb.DpfKey()
        k0.ParseFromString(a)
        k1.ParseFromString(b)
        return k0, k1

    def create_evaluation_context(self, key: pb.DpfKey) -> pb.EvaluationContext:
        ctx = pb.EvaluationContext()
        ctx.ParseFromString(_call(self._impl.create_evaluation_context, key.SerializeToString()))
        return ctx

    # -- evaluation (GPU) ----------------------------------------------------
    def _type(self, h, value_type):
        if value_type is not None:
            return value_type
        return self._parameters[h].value_type if 0 <= h < len(self._parameters) else None

    def evaluate_until(self, hierarchy_level: int, prefixes: Sequence[int],
                       ctx: pb.EvaluationContext, value_type: Optional[pb.ValueType] = None,
                       packed: bool = False) -> np.ndarray:
        vt_bytes = value_type.SerializeToString() if value_type is not None else None
        out, new_ctx = _call(self._impl.evaluate_until, int(hierarchy_level), u128_array(prefixes),
                             ctx.SerializeToString(), vt_bytes)
        ctx.ParseFromString(new_ctx)
        vt = self._type(hierarchy_level, value_type)
        size = sum(b // 8 for _, b, _ in leaves_of(vt))
        n = out.size // size
        return out.reshape(n, size) if packed else _natural(vt, out, n)

    def evaluate_next(self, prefixes: Sequence[int], ctx: pb.EvaluationContext, **kw):
        if len(prefixes) == 0:
            return self.evaluate_until(0, prefixes, ctx, **kw)
        return self.evaluate_until(ctx.previous_hierarchy_level + 1, prefixes, ctx, **kw)

    def evaluate_at(self, key_or_level, level_or_points, points=None, ctx=None,
                    value_type: Optional[pb.ValueType] = None, packed: bool = False):
        """evaluate_at(key, level, points)  or  evaluate_at(level, points, ctx=ctx)
        (the two overloads of h:331-360)."""
        vt_bytes = value_type.SerializeToString() if value_type is not None else None
        if isinstance(key_or_level, pb.DpfKey):
            key, h, pts = key_or_level, int(level_or_points), points
            out = _call(self._impl.evaluate_at, key.SerializeToString(), h, u128_array(pts),
                        vt_bytes)
        else:
            h, pts = int(key_or_level), level_or_points
            if ctx is None:
                ctx = points
            out, new_ctx = _call(self._impl.evaluate_at_ctx, h, u128_array(pts),
                                 ctx.SerializeToString(), vt_bytes)
            ctx.ParseFromString(new_ctx)
        vt = self._type(h, value_type)
        size = sum(b // 8 for _, b, _ in leaves_of(vt))
        n = out.size // size
        return out.reshape(n, size) if packed else _natural(vt, out, n)

    # -- MI355X extensions -----------------------------------------------------
    def evaluate_until_to_device(self, hierarchy_level: int, prefixes: Sequence[int],
                                 ctx: pb.EvaluationContext, out, stream=None) -> int:
        """Writes packed outputs into the torch device tensor `out`; returns the
        number of elements.  `stream`: a torch.cuda.Stream (default: current)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        n, new_ctx = _call(self._impl.evaluate_until_to_device, int(hierarchy_level),
                           u128_array(prefixes), ctx.SerializeToString(), out.data_ptr(),
                           out.numel() * out.element_size(), s.cuda_stream, None)
        ctx.ParseFromString(new_ctx)
        return n

    def evaluate_shard_to_device(self, hierarchy_level: int, shard: int, num_shards: int,
                                 ctx: pb.EvaluationContext, out, stream=None) -> int:
        """Full-domain evaluation of one subtree-prefix shard into device tensor `out`."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        n, new_ctx = _call(self._impl.evaluate_shard_to_device, int(hierarchy_level), int(shard),
                           int(num_shards), ctx.SerializeToString(), out.data_ptr(),
                           out.numel() * out.element_size(), s.cuda_stream)
        ctx.ParseFromString(new_ctx)
        return n

    def evaluate_dot_to_device(self, key: pb.DpfKey, hierarchy_level: int, db, record_words: int,
                               out, shard: int = 0, num_shards: int = 1, stream=None) -> int:
        """Two-server PIR answer: full-domain evaluation of `key` folded into the
        database `db` (torch device tensor: this shard's records, row-major,
        `record_words` words of the value type's width each) without storing
        the share vector.  Writes `record_words` packed elements into the torch
        device tensor `out`: sum_i y[i] * db[i][w] mod 2^64 for uint64,
        XOR_i (y[i] & db[i][w]) for XorWrapper<uint64 / uint128>.  The two
        parties' (and all shards') results combine with the type's +."""
        s = stream
        if s is None:
            import torch
            s = torch.cuda.current_stream(out.device)
        return _call(self._impl.evaluate_dot_to_device, key.SerializeToString(),
                     int(hierarchy_level), int(shard), int(num_shards), db.data_ptr(),
                     db.numel() * db.element_size(), int(record_words), out.data_ptr(),
                     out.numel() * out.element_size(), s.cuda_stream)

    def evaluate_dot(self, key: pb.DpfKey, hierarchy_level: int, db, record_words: int):
        """evaluate_dot_to_device over the whole domain, returned as numpy
        (uint64 per word; (record_words, 16) bytes for 128-bit words)."""
        out = _call(self._impl.evaluate_dot, key.SerializeToString(), int(hierarchy_level),
                    db.data_ptr(), db.numel() * db.element_size(), int(record_words))
        return _natural(self._parameters[hierarchy_level].value_type, out, int(record_words))

    def evaluate_select_to_device(self, keys: Sequence[pb.DpfKey], hierarchy_level: int, db,
                                  record_words: int, out, shard: int = 0, num_shards: int = 1,
                                  stream=None) -> int:
        """Dense two-server PIR answers of up to 64 keys against one pass over
        the database: for XorWrapper<uint64 / uint128> every output *bit* of a
        key's full-domain evaluation selects one record (128 per leaf block),
        and out[q][w] = XOR of db[j][w] over the set bits j of key q.  `db`
        (torch device tensor) holds this shard's records, row-major,
        `record_words` uint64 words each; writes len(keys) * record_words
        uint64 into the torch device tensor `out` and returns that count.  The
        two parties' (and all shards') answers combine with XOR."""
        s = stream
        if s is None:
            import torch
            s = torch.cuda.current_stream(out.device)
        return _call(self._impl.evaluate_select_to_device,
                     [k.SerializeToString() for k in keys], int(hierarchy_level), int(shard),
                     int(num_shards), db.data_ptr(), db.numel() * db.element_size(),
                     int(record_words), out.data_ptr(), out.numel() * out.element_size(),
                     s.cuda_stream)

    def evaluate_select(self, keys: Sequence[pb.DpfKey], hierarchy_level: int, db,
                        record_words: int, shard: int = 0, num_shards: int = 1):
        """evaluate_select_to_device returned as a numpy uint64 array of shape
        (len(keys), record_words)."""
        if int(num_shards) == 1 and int(shard) == 0:
            return _call(self._impl.evaluate_select, [k.SerializeToString() for k in keys],
                         int(hierarchy_level), db.data_ptr(), db.numel() * db.element_size(),
                         int(record_words))
        import torch
        n = max(len(keys) * int(record_words), 0)
        out = torch.empty(max(n, 1), dtype=torch.int64, device=db.device)
        self.evaluate_select_to_device(keys, hierarchy_level, db, record_words, out, shard=shard,
                                       num_shards=num_shards)
        torch.cuda.synchronize(out.device)
        return out[:n].cpu().numpy().view(np.uint64).reshape(len(keys), int(record_words))

    def evaluate_dot_batch_to_device(self, keys: Sequence[pb.DpfKey], hierarchy_level: int, db,
                                     record_words: int, out, shard: int = 0, num_shards: int = 1,
                                     stream=None) -> int:
        """Additive-share two-server PIR answers of up to 64 keys against one
        pass over the database: evaluate_dot_to_device for every key at once,
        for uint64 (out[q][w] = sum_i y_q[i] * db[i][w] mod 2^64) and
        XorWrapper<uint64> (XOR_i (y_q[i] & db[i][w])).  `db` (torch device
        tensor) holds this shard's records, row-major, `record_words` uint64
        words each; writes len(keys) * record_words uint64 into the torch
        device tensor `out` and returns that count.  The two parties' (and all
        shards') answers combine with the type's +."""
        s = stream
        if s is None:
            import torch
            s = torch.cuda.current_stream(out.device)
        return _call(self._impl.evaluate_dot_batch_to_device,
                     [k.SerializeToString() for k in keys], int(hierarchy_level), int(shard),
                     int(num_shards), db.data_ptr(), db.numel() * db.element_size(),
                     int(record_words), out.data_ptr(), out.numel() * out.element_size(),
                     s.cuda_stream)

    def evaluate_dot_batch(self, keys: Sequence[pb.DpfKey], hierarchy_level: int, db,
                           record_words: int, shard: int = 0, num_shards: int = 1):
        """evaluate_dot_batch_to_device returned as a numpy uint64 array of
        shape (len(keys), record_words)."""
        if int(num_shards) == 1 and int(shard) == 0:
            return _call(self._impl.evaluate_dot_batch, [k.SerializeToString() for k in keys],
                         int(hierarchy_level), db.data_ptr(), db.numel() * db.element_size(),
                         int(record_words))
        import torch
        n = max(len(keys) * int(record_words), 0)
        out = torch.empty(max(n, 1), dtype=torch.int64, device=db.device)
        self.evaluate_dot_batch_to_device(keys, hierarchy_level, db, record_words, out,
                                          shard=shard, num_shards=num_shards)
        torch.cuda.synchronize(out.device)
        return out[:n].cpu().numpy().view(np.uint64).reshape(len(keys), int(record_words))

    def evaluate_at_batch(self, keys: Sequence[pb.DpfKey], hierarchy_level: int,
                          points: Sequence[int], points_per_key: int, packed: bool = False):
        pts = points if isinstance(points, np.ndarray) else u128_array(points)
        out = _call(self._impl.evaluate_at_batch, [k.SerializeToString() for k in keys],
                    int(hierarchy_level), pts, int(points_per_key))
        vt = self._parameters[hierarchy_level].value_type
        size = sum(b // 8 for _, b, _ in leaves_of(vt))
        n = out.size // size
        return out.reshape(n, size) if packed else _natural(vt, out, n)

    # -- key batches -------------------
    def make_key_batch(self, keys: Sequence[pb.DpfKey]):
        """SoA image of `keys` (host); .upload(begin, end, stream) puts rows on the GPU."""
        return _call(self._impl.make_key_batch, [k.SerializeToString() for k in keys])

    def parse_key_batch(self, serialized_keys: Sequence[bytes], threads: int = 0):
        """SoA key batch straight from serialized DpfKeys, parsed and validated
        on host threads (batched key ingestion)."""
        return _call(self._impl.parse_key_batch, list(serialized_keys), int(threads))

    def serialize_key_batch(self, batch, threads: int = 0) -> List[bytes]:
        """Every row of a key batch as a serialized DpfKey (inverse of
        parse_key_batch), on host threads."""
        return _call(self._impl.serialize_key_batch, batch, int(threads))

    def key_from_batch(self, batch, k: int) -> pb.DpfKey:
        key = pb.DpfKey()
        key.ParseFromString(_call(self._impl.key_from_batch, batch, int(k)))
        return key

    def generate_key_batch(self, alphas: Sequence[int], beta: Sequence,
                           root_seeds: Optional[np.ndarray] = None, threads: int = 0):
        """Both parties' key batches for every alpha (shared beta per hierarchy
        level), generated on `threads` host threads.  root_seeds: uint64 (2n, 2)
        array ({low, high} per seed, two per key) or None for fresh randomness."""
        al = alphas if isinstance(alphas, np.ndarray) else u128_array(alphas)
        return _call(self._impl.generate_key_batch, al, self._betas(beta), root_seeds, int(threads))

    def generate_key_batch_with_betas(self, alphas: Sequence[int], betas: Sequence,
                                      root_seeds: Optional[np.ndarray] = None, threads: int = 0):
        """generate_key_batch with a beta of its own for every key: `betas` holds
        len(alphas) * H values, key-major."""
        al = alphas if isinstance(alphas, np.ndarray) else u128_array(alphas)
        return _call(self._impl.generate_key_batch_with_betas, al, self._betas(betas), root_seeds,
                     int(threads))

    def generate_key_batch_to_device(self, alphas: Sequence[int], beta: Sequence,
                                     root_seeds: Optional[np.ndarray] = None, stream=None):
        """Both parties' key batches generated in device memory on `stream`:
        the same bytes as generate_key_batch (H betas) or
        generate_key_batch_with_betas (len(alphas) * H betas) followed by an
        upload.  Runs the key generation kernel where
        generates_keys_on_device(), else generates on the host and uploads."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        al = alphas if isinstance(alphas, np.ndarray) else u128_array(alphas)
        return _call(self._impl.generate_key_batch_to_device, al, self._betas(beta), root_seeds,
                     s.cuda_stream)

    def generates_keys_on_device(self) -> bool:
        """Whether generate_key_batch_to_device runs on the GPU (every level's
        value type is one integer or XorWrapper leaf) or falls back to the host."""
        return self._impl.generates_keys_on_device()

    def download_key_batch(self, device_batch, stream=None):
        """The host image of a device key batch (inverse of upload_key_batch)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return _call(device_batch.download, s.cuda_stream)

    def upload_key_batch(self, batch, begin: int = 0, end: Optional[int] = None, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        end = batch.num_keys if end is None else end
        return _call(batch.upload, int(begin), int(end), s.cuda_stream)

    def evaluate_at_batch_to_device(self, device_batch, hierarchy_level: int, points,
                                    points_per_key: int, out, shared_points: bool = False,
                                    stream=None) -> int:
        """EvaluateAt for every key of a device batch at device points (a torch
        int64 tensor (n, 2) of {low, high}); packed outputs [key][point] in `out`."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        return _call(self._impl.evaluate_at_batch_to_device, device_batch, int(hierarchy_level),
                     points.data_ptr(), int(points_per_key), bool(shared_points), out.data_ptr(),
                     out.numel() * out.element_size(), s.cuda_stream)

    def evaluate_at_batch_sum_to_device(self, device_batch, hierarchy_level: int, points, out,
                                        stream=None) -> None:
        """out[j] = group sum over the batch's keys of EvaluateAt(key, points[j])."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        _call(self._impl.evaluate_at_batch_sum_to_device, device_batch, int(hierarchy_level),
              points.data_ptr(), int(points.shape[0]), out.data_ptr(), s.cuda_stream)

    def evaluate_lookup_batch_to_device(self, device_batch, hierarchy_level: int, offsets, table,
                                        table_words: int, out, stream=None) -> int:
        """Private table lookup for every key of a device batch: the key's
        full-domain evaluation y_k (uint64 or XorWrapper<uint64>, 2^n elements)
        folded into the shared public `table` (torch device tensor, 2^n rows
        of `table_words` uint64, row-major) rotated by the key's public offset
        s_k = offsets[k] mod 2^n (`offsets`: torch device tensor of K uint64 or
        int64), without storing y_k:
        out[k][w] = sum_i y_k[i] * T[(i + s_k) mod 2^n][w] mod 2^64, or
        XOR_i (y_k[i] & T[...][w]).  Writes K * table_words uint64 into the
        torch device tensor `out` and returns that count.  The two parties'
        results add (XOR) to beta_k * T[(alpha_k + s_k) mod 2^n]."""
        s = stream
        if s is None:
            import torch
            s = torch.cuda.current_stream(out.device)
        return _call(self._impl.evaluate_lookup_batch_to_device, device_batch,
                     int(hierarchy_level), offsets.data_ptr(), table.data_ptr(),
                     table.numel() * table.element_size(), int(table_words), out.data_ptr(),
                     out.numel() * out.element_size(), s.cuda_stream)

    def evaluate_lookup_batch(self, device_batch, hierarchy_level: int, offsets, table,
                              table_words: int) -> np.ndarray:
        """evaluate_lookup_batch_to_device with host offsets, returned as a numpy
        uint64 array of shape (K, table_words)."""
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        out = _call(self._impl.evaluate_lookup_batch, device_batch, int(hierarchy_level), off,
                    table.data_ptr(), table.numel() * table.element_size(), int(table_words))
        return out.reshape(-1, int(table_words))

    def evaluates_lookup_on_device(self, hierarchy_level: int) -> bool:
        """Whether evaluate_lookup_batch_to_device takes this level's value type
        and domain size (there is no fallback behind it)."""
        return self._impl.evaluates_lookup_on_device(int(hierarchy_level))

    def check_lookup_args(self, num_keys: int, hierarchy_level: int, offsets, table,
                          table_words: int, out, batch_matches: bool = True) -> None:
        """The host checks of evaluate_lookup_batch_to_device for a batch of
        `num_keys` keys, in its order; raises what it would raise.  Touches no
        device and needs no batch."""
        _call(self._impl.check_lookup_args, int(num_keys), bool(batch_matches),
              int(hierarchy_level), offsets.data_ptr(), table.data_ptr(),
              table.numel() * table.element_size(), int(table_words), out.data_ptr(),
              out.numel() * out.element_size())

    def evaluate_dot_buckets_to_device(self, device_batch, hierarchy_level: int, bucket_begin, db,
                                       record_words: int, out, stream=None) -> int:
        """Multi-query PIR over a bucketed database: every key of a device batch
        expanded over its domain (uint64 or XorWrapper<uint64>, N = 2^n
        elements, n <= 24) and folded into its own bucket's slice of `db` (torch
        device tensor [B][N][record_words] of uint64, row-major).  Keys
        bucket_begin[b] .. bucket_begin[b + 1] - 1 belong to bucket b
        (`bucket_begin`: B + 1 host integers from 0 to K, nondecreasing):
        out[k][w] = sum_i y_k[i] * db[b(k)][i][w] mod 2^64, or
        XOR_i (y_k[i] & db[b(k)][i][w]).  Writes K * record_words uint64 into
        the torch device tensor `out` and returns that count.  The two
        parties' rows add (XOR) to beta_k * db[b(k)][alpha_k]."""
        s = stream
        if s is None:
            import torch
            s = torch.cuda.current_stream(out.device)
        return _call(self._impl.evaluate_dot_buckets_to_device, device_batch,
                     int(hierarchy_level), [int(x) for x in bucket_begin], db.data_ptr(),
                     db.numel() * db.element_size(), int(record_words), out.data_ptr(),
                     out.numel() * out.element_size(), s.cuda_stream)

    def evaluate_dot_buckets(self, device_batch, hierarchy_level: int, bucket_begin, db,
                             record_words: int) -> np.ndarray:
        """evaluate_dot_buckets_to_device returned as a numpy uint64 array of
        shape (K, record_words)."""
        out = _call(self._impl.evaluate_dot_buckets, device_batch, int(hierarchy_level),
                    [int(x) for x in bucket_begin], db.data_ptr(),
                    db.numel() * db.element_size(), int(record_words))
        return out.reshape(-1, int(record_words))

    def evaluates_dot_buckets_on_device(self, hierarchy_level: int) -> bool:
        """Whether evaluate_dot_buckets_to_device takes this level's value type
        and domain size (there is no fallback behind it)."""
        return self._impl.evaluates_dot_buckets_on_device(int(hierarchy_level))

    def check_dot_buckets_args(self, num_keys: int, hierarchy_level: int, bucket_begin, db,
                               record_words: int, out, batch_matches: bool = True) -> None:
        """The host checks of evaluate_dot_buckets_to_device for a batch of
        `num_keys` keys, in its order; raises what it would raise.  Touches no
        device and needs no batch."""
        _call(self._impl.check_dot_buckets_args, int(num_keys), bool(batch_matches),
              int(hierarchy_level), [int(x) for x in bucket_begin], db.data_ptr(),
              db.numel() * db.element_size(), int(record_words), out.data_ptr(),
              out.numel() * out.element_size())

    def evaluate_full_domain_sum_to_device(self, device_batch, hierarchy_level: int, out,
                                           accumulate: bool = False, stream=None) -> int:
        """Private histogram of a device batch: every key's full-domain
        evaluation y_k (uint64 or XorWrapper<uint64>, N = 2^n elements, n <= 30)
        summed element by element without storing y_k,
        out[i] = sum_k y_k[i] mod 2^64, or XOR_k y_k[i].  `out`: a torch device
        tensor of at least N 64-bit words, 16-byte aligned; overwritten, or with
        `accumulate` added (XORed) into.  Returns N.  The two parties' vectors
        add (XOR) to sum_k beta_k * e_{alpha_k}."""
        s = stream
        if s is None:
            import torch
            s = torch.cuda.current_stream(out.device)
        return _call(self._impl.evaluate_full_domain_sum_to_device, device_batch,
                     int(hierarchy_level), out.data_ptr(), out.numel() * out.element_size(),
                     bool(accumulate), s.cuda_stream)

    def evaluate_full_domain_sum(self, device_batch, hierarchy_level: int) -> np.ndarray:
        """evaluate_full_domain_sum_to_device into a fresh vector, returned as a
        numpy uint64 array of N sums."""
        return _call(self._impl.evaluate_full_domain_sum, device_batch, int(hierarchy_level))

    def evaluates_full_domain_sum_on_device(self, hierarchy_level: int) -> bool:
        """Whether evaluate_full_domain_sum_to_device takes this level's value
        type and domain size (there is no fallback behind it)."""
        return self._impl.evaluates_full_domain_sum_on_device(int(hierarchy_level))

    def check_full_domain_sum_args(self, num_keys: int, hierarchy_level: int, out,
                                   batch_matches: bool = True) -> None:
        """The host checks of evaluate_full_domain_sum_to_device for a batch of
        `num_keys` keys, in its order; raises what it would raise.  Touches no
        device and needs no batch."""
        _call(self._impl.check_full_domain_sum_args, int(num_keys), bool(batch_matches),
              int(hierarchy_level), out.data_ptr(), out.numel() * out.element_size())

    def evaluate_full_domain_sum_packed_to_device(self, device_batch, hierarchy_level: int, out,
                                                  accumulate: bool = False, stream=None) -> int:
        """evaluate_full_domain_sum_to_device for every integer width whose
        elements fill a leaf block: uint8/16/32/64 summed mod 2^B, XorWrapper of
        8 to 128 bits XORed.  `out`: a torch device tensor of at least N = 2^n
        packed elements (N * B / 8 bytes, the layout evaluate_until writes),
        16-byte aligned; overwritten, or with `accumulate` added (XORed) into
        element by element.  Returns N.  The 64-bit types give
        evaluate_full_domain_sum_to_device's bytes; everything else the level
        could be is UNIMPLEMENTED."""
        s = stream
        if s is None:
            import torch
            s = torch.cuda.current_stream(out.device)
        return _call(self._impl.evaluate_full_domain_sum_packed_to_device, device_batch,
                     int(hierarchy_level), out.data_ptr(), out.numel() * out.element_size(),
                     bool(accumulate), s.cuda_stream)

    def evaluate_full_domain_sum_packed(self, device_batch, hierarchy_level: int) -> np.ndarray:
        """evaluate_full_domain_sum_packed_to_device into a fresh vector,
        returned as a numpy uint8, uint16, uint32 or uint64 array of N elements,
        or uint64 (N, 2) (low word first) for 128 bits."""
        raw = _call(self._impl.evaluate_full_domain_sum_packed, device_batch, int(hierarchy_level))
        size = self.packed_size(int(hierarchy_level))
        if size == 16:
            return raw.view(np.uint64).reshape(-1, 2)
        return raw.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[size])

    def evaluates_full_domain_sum_packed_on_device(self, hierarchy_level: int) -> bool:
        """Whether evaluate_full_domain_sum_packed_to_device takes this level's
        value type, domain size and tree level (there is no fallback behind
        it)."""
        return self._impl.evaluates_full_domain_sum_packed_on_device(int(hierarchy_level))

    def check_full_domain_sum_packed_args(self, num_keys: int, hierarchy_level: int, out,
                                          batch_matches: bool = True) -> None:
        """The host checks of evaluate_full_domain_sum_packed_to_device for a
        batch of `num_keys` keys, in its order; raises what it would raise.
        Touches no device and needs no batch."""
        _call(self._impl.check_full_domain_sum_packed_args, int(num_keys), bool(batch_matches),
              int(hierarchy_level), out.data_ptr(), out.numel() * out.element_size())

    def evaluate_full_domain_sum_sketch_to_device(self, hierarchy_level: int, device_batch,
                                                  weights, sum_out, sketch_out=None,
                                                  accumulate: bool = False, stream=None) -> int:
        """Checked private histogram of a device batch over a field
        (IntModN<uint32, N_0> or a 2-tuple of such, nl leaves, N = 2^n elements,
        n <= 28): sum_out[i][e] = sum_k y_k[i][e] mod N_e and, for the J <= 2 rows
        of `weights` (torch device tensor, J x N 32-bit words, or None for J = 0),
        sketch_out[k][j][e] = sum_i (w[j][i] mod N_e) * y_k[i][e] mod N_e, in
        one launch that stores no y_k.  `sum_out`: at least N * nl 32-bit words,
        16-byte aligned; overwritten, or with `accumulate` added into mod N_e
        (its entries must be below N_e).  `sketch_out`: at least K * J * nl
        words, always overwritten.  Returns N."""
        s = stream
        if s is None:
            import torch
            s = torch.cuda.current_stream(sum_out.device)
        J = 0 if weights is None else int(weights.shape[0]) if weights.dim() > 1 else 1
        nbytes = lambda t: 0 if t is None else t.numel() * t.element_size()
        ptr = lambda t: 0 if t is None else t.data_ptr()
        return _call(self._impl.evaluate_full_domain_sum_sketch_to_device, int(hierarchy_level),
                     device_batch, ptr(weights), J, ptr(sum_out), nbytes(sum_out),
                     ptr(sketch_out), nbytes(sketch_out), bool(accumulate), s.cuda_stream)

    def evaluate_full_domain_sum_sketch(self, hierarchy_level: int, device_batch, weights=None):
        """evaluate_full_domain_sum_sketch_to_device with host weights (J x N,
        None: J = 0) into fresh arrays: numpy uint32 (sums [N, nl], sketches
        [K, J, nl])."""
        w = (np.zeros((0, 0), dtype=np.uint32) if weights is None
             else np.ascontiguousarray(weights, dtype=np.uint32))
        J = int(w.shape[0]) if w.ndim > 1 else 1
        sums, sk = _call(self._impl.evaluate_full_domain_sum_sketch, int(hierarchy_level),
                         device_batch, w.reshape(-1), J)
        n = int(self.parameters()[hierarchy_level].log_domain_size)
        nl = sums.size >> n
        return sums.reshape(1 << n, nl), sk.reshape(int(device_batch.num_keys), J, nl)

    def evaluates_full_domain_sum_sketch_on_device(self, hierarchy_level: int) -> bool:
        """Whether evaluate_full_domain_sum_sketch_to_device takes this level's
        value type and domain size (there is no fallback behind it)."""
        return self._impl.evaluates_full_domain_sum_sketch_on_device(int(hierarchy_level))

    def check_full_domain_sum_sketch_args(self, num_keys: int, hierarchy_level: int, weights,
                                          num_weight_rows: int, sum_out, sketch_out,
                                          batch_matches: bool = True) -> None:
        """The host checks of evaluate_full_domain_sum_sketch_to_device for a
        batch of `num_keys` keys, in its order; raises what it would raise.
        Touches no device and needs no batch.  Each buffer is None or a
        (address, bytes) pair."""
        w, s, k = (b if b is not None else (0, 0) for b in (weights, sum_out, sketch_out))
        _call(self._impl.check_full_domain_sum_sketch_args, int(num_keys), bool(batch_matches),
              int(hierarchy_level), int(w[0]), int(num_weight_rows), int(s[0]), int(s[1]),
              int(k[0]), int(k[1]))

    # -- device-resident incremental evaluation of a key batch (8f.1, cfg 5b) --
    def create_batch_evaluation_context(self, device_batch):
        """EvaluationContext of every key of a device batch, kept on the GPU."""
        return _call(self._impl.create_batch_evaluation_context, device_batch)

    def evaluate_until_batch_to_device(self, hierarchy_level: int, prefixes, batch_ctx, out,
                                       sum_over_keys: bool = False, stream=None) -> int:
        """EvaluateUntil(hierarchy_level, prefixes, ctx_k) for every key k of the
        batch (same prefixes for all keys).  Packed outputs go to the torch
        device tensor `out`: [key][element], or with `sum_over_keys` the group
        sum over keys [element].  Returns the elements per key."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        pre = prefixes if isinstance(prefixes, np.ndarray) else u128_array(prefixes)
        return _call(self._impl.evaluate_until_batch_to_device, int(hierarchy_level), pre,
                     batch_ctx, bool(sum_over_keys), out.data_ptr(),
                     out.numel() * out.element_size(), s.cuda_stream)

    def evaluate_until_batch_sketch_to_device(self, hierarchy_level: int, prefixes, batch_ctx,
                                              weights, sketch_out, sums_out=None,
                                              stream=None) -> int:
        """evaluate_until_batch_to_device with every key's linear sketch of its
        own output vector y_k (n elements of nl IntModN<uint32, N_e> leaves):
        `weights` is a torch device tensor of uint32 bits, shape (J, n) with
        1 <= J <= 4 (any 32-bit values), and
        sketch_out[k][j][e] = (sum_i (weights[j][i] mod N_e) * y_k[i][e]) mod N_e
        is written as K * J * nl uint32 into the torch device tensor
        `sketch_out`.  With `sums_out`, it also receives what sum_over_keys
        writes.  The context is left as that call leaves it.  Returns n."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(sketch_out.device)
        pre = prefixes if isinstance(prefixes, np.ndarray) else u128_array(prefixes)
        if weights.dim() != 2 or weights.element_size() != 4 or not weights.is_contiguous():
            raise ValueError("weights must be a contiguous (J, n) tensor of 32-bit elements")
        return _call(self._impl.evaluate_until_batch_sketch_to_device, int(hierarchy_level), pre,
                     batch_ctx, weights.data_ptr(), int(weights.shape[0]), int(weights.shape[1]),
                     sums_out.data_ptr() if sums_out is not None else 0,
                     sums_out.numel() * sums_out.element_size() if sums_out is not None else 0,
                     sketch_out.data_ptr(), sketch_out.numel() * sketch_out.element_size(),
                     s.cuda_stream)

    def evaluate_next_batch_to_device(self, prefixes, batch_ctx, out, sum_over_keys: bool = False,
                                      stream=None) -> int:
        """EvaluateNext for every key of the batch (h:363-365)."""
        level = 0 if len(prefixes) == 0 else batch_ctx.previous_hierarchy_level + 1
        return self.evaluate_until_batch_to_device(level, prefixes, batch_ctx, out,
                                                   sum_over_keys, stream)

    def export_evaluation_context(self, batch_ctx, host_batch, k: int,
                                  stream=None) -> pb.EvaluationContext:
        """Key k's context as the EvaluationContext proto EvaluateUntil leaves."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        ctx = pb.EvaluationContext()
        ctx.ParseFromString(_call(self._impl.export_evaluation_context, batch_ctx, host_batch,
                                  int(k), s.cuda_stream))
        return ctx

    def sum_packed_shares(self, hierarchy_level: int, shares: np.ndarray, num_shares: int,
                          count: int) -> np.ndarray:
        """Group sum of num_shares packed vectors of `count` elements (host)."""
        return _call(self._impl.sum_packed_shares, int(hierarchy_level),
                     np.ascontiguousarray(shares, dtype=np.uint8).reshape(-1), int(num_shares),
                     int(count))

    def packed_size(self, h: int) -> int:
        return self._impl.packed_size(h)

    def output_elements(self, h: int, num_prefixes: int, previous_hierarchy_level: int) -> int:
        """Elements EvaluateUntil(h, prefixes) returns for len(prefixes) == num_prefixes."""
        return _call(self._impl.output_elements, int(h), int(num_prefixes),
                     int(previous_hierarchy_level))

    def tree_levels_needed(self) -> int:
        return self._impl.tree_levels_needed()

    def hierarchy_to_tree(self) -> List[int]:
        return list(self._impl.hierarchy_to_tree())

    def blocks_needed(self, h: int) -> int:
        return self._impl.blocks_needed(h)
