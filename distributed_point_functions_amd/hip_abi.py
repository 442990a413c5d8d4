"""ctypes binding of the C ABI in ``include/dpf_hip.h`` (``lib/libdpf_hip.so``).

Device buffers are torch tensors (torch is plumbing here: device memory,
streams, ``torch.distributed``); every compute call goes to the hand-written
gfx950 kernels.  There is no CPU fallback: if the shared library is missing
or no GPU is visible, calls raise.

torch is imported *before* the library is loaded so that both share one HIP
runtime (torch ships ``libamdhip64.so.7`` with the same SONAME).
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPF_HIP_LIB") or os.path.join(_HERE, "lib", "libdpf_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "dpf_hip.h")
MAX_LEAVES = 16
LEAF_INT, LEAF_INTMODN, LEAF_XOR = 0, 1, 2
MASK64 = (1 << 64) - 1

_lib = None


class DpfHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class Block(ctypes.Structure):
    _fields_ = [("low", ctypes.c_uint64), ("high", ctypes.c_uint64)]


class AesKey(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_uint8 * 16)]


class ValueDesc(ctypes.Structure):
    _fields_ = [
        ("num_leaves", ctypes.c_int32),
        ("direct", ctypes.c_int32),
        ("elements_per_block", ctypes.c_int32),
        ("blocks_needed", ctypes.c_int32),
        ("kind", ctypes.c_int32 * MAX_LEAVES),
        ("bits", ctypes.c_int32 * MAX_LEAVES),
        ("mod_low", ctypes.c_uint64 * MAX_LEAVES),
        ("mod_high", ctypes.c_uint64 * MAX_LEAVES),
    ]


class PrefixBatchArgs(ctypes.Structure):
    """dpf_prefix_batch_args, member by member; prefix_batch_args() makes one."""
    _P, _I, _I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_keys", _I64), ("num_starts", _I64),
                ("walk_levels", _I), ("save_after", _I), ("expand_levels", _I), ("cw_first", _I),
                ("cw_stride", _I), ("key_seed", _P), ("party", _P), ("seeds_in", _P),
                ("control_in", _P), ("in_stride", _I64), ("parent", _P), ("path", _P),
                ("save_index", _P), ("seeds_out", _P), ("control_out", _P), ("out_stride", _I64),
                ("cw_seed", _P), ("cw_left", _P), ("cw_right", _P),
                ("key_left", ctypes.POINTER(AesKey)), ("key_right", ctypes.POINTER(AesKey)),
                ("key_value", ctypes.POINTER(AesKey)), ("desc", ctypes.POINTER(ValueDesc)),
                ("elements_per_leaf", _I), ("value_correction", _P), ("sum", _I),
                ("workspace", _P), ("out", _P), ("leaf_cache", _P), ("leaf_stride", _I64),
                ("leaf_slot", _P), ("index_major", _I), ("num_weights", _I),
                ("slot_weights", _P), ("accumulators", _P), ("sketch", _P)]


def prefix_batch_args(**members) -> PrefixBatchArgs:
    """A zeroed dpf_prefix_batch_args with struct_size and `members` set (keys
    and descriptor as ctypes.pointer(...), device pointers as integers)."""
    a = PrefixBatchArgs(**members)
    a.struct_size = ctypes.sizeof(PrefixBatchArgs)
    return a


def header_functions() -> list:
    """Names of every function the C ABI header declares."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(dpf_hip_\w+)\s*\(", txt, re.M)))


def load(require_gpu: bool = False):
    """Loads libdpf_hip.so (after torch, to share its HIP runtime)."""
    global _lib
    if _lib is None:
        try:
            import torch  # noqa: F401  (shared HIP runtime)
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise DpfHipError(13, f"HIP extension not built: {LIB_PATH} "
                                  "(run python -m distributed_point_functions_amd.build_native)")
        L = ctypes.CDLL(LIB_PATH)
        P, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.dpf_hip_last_error.restype = ctypes.c_char_p
        L.dpf_hip_last_expand_kernel.restype = ctypes.c_char_p
        L.dpf_hip_last_expand_kernel.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.dpf_hip_last_batch_kernel.restype = ctypes.c_char_p
        L.dpf_hip_last_batch_kernel.argtypes = []
        L.dpf_hip_last_points_kernel.restype = ctypes.c_char_p
        L.dpf_hip_last_points_kernel.argtypes = []
        L.dpf_hip_hash.argtypes = [I64, P, P, P, P]
        L.dpf_hip_eval_paths.argtypes = [I64, I, P, P, P, P, P, P, P, P, P, P, P]
        L.dpf_hip_expand.argtypes = [I64, P, P, I, P, P, P, P, P, P, P, I, P, I, P, P]
        L.dpf_hip_eval_points.argtypes = [I64, I64, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P,
                                          P, P]
        L.dpf_hip_gather.argtypes = [I64, I64, I, P, P, P, P]
        L.dpf_hip_sum_shares_u64.argtypes = [I64, I64, I, I, P, P, P]
        L.dpf_hip_packed_element_size.argtypes = [P]
        L.dpf_hip_event_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        L.dpf_hip_event_destroy.argtypes = [P]
        L.dpf_hip_event_record.argtypes = [P, P]
        L.dpf_hip_event_elapsed_ms.argtypes = [P, P, ctypes.POINTER(ctypes.c_float)]
        L.dpf_hip_stream_sync.argtypes = [P]
        L.dpf_hip_clock_probe.argtypes = [I]
        L.dpf_hip_clock_probe_read.argtypes = [ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_int64),
                                               ctypes.POINTER(ctypes.c_double)]
        # Entry points a parent build swapped in for an A/B (tools/ab.sh lib:<name>)
        # may not have yet; build() checks the in-tree library for every symbol.
        for name, types in (("dpf_hip_clock_probe_exits", [ctypes.POINTER(ctypes.c_double)]),
                            ("dpf_hip_octet_schedule",
                             [I64, I, I, I, I, ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_last_expand_schedule", [ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_last_dynamic_chunks", [ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_mic_eval_batch",
                             [I64, I, P, P, P, P, P, I, P, P, I, P, I] + [P] * 11),
                            ("dpf_hip_expand_dot",
                             [I64, P, P, I, P, P, P, P, P, P, P, I, P, I, P, I, P, P, P]),
                            ("dpf_hip_dot_rows", [I64, I, P, P, P, I, P, P, P]),
                            ("dpf_hip_expand_dot_workspace_bytes", [P, I]),
                            ("dpf_hip_expand_dot_fused", [P, I]),
                            ("dpf_hip_last_dot_kernel", []),
                            ("dpf_hip_select_rows", [I64, I, I, P, I64, P, I, P, P, P]),
                            ("dpf_hip_select_workspace_bytes", [I, I]),
                            ("dpf_hip_last_select_shape", [ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_dot_rows_batch", [I64, I, I, P, P, I64, P, I, P, P, P]),
                            ("dpf_hip_dot_rows_batch_workspace_bytes", [P, I, I]),
                            ("dpf_hip_last_dot_batch_shape", [ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_sketch_rows", [I64, I64, P, P, I, I, P, P, P]),
                            ("dpf_hip_sketch_supported", [P]),
                            ("dpf_hip_gen_keys_supported", [P]),
                            ("dpf_hip_gen_key_batch",
                             [I64, I, I, P, P, P, P, P, P, P, I, I, P, P, P, P, P, P, P, P]),
                            ("dpf_hip_prefix_batch_sketch_fused", [P, I, I, I, I, I, I]),
                            ("dpf_hip_sketch_slot_weights", [I64, I64, P, P, I, P, P, P]),
                            ("dpf_hip_dcf_expand_supported", [P, I, P]),
                            ("dpf_hip_dcf_expand",
                             [I64, I, I, I64, P, P, P, P, P, I, P, P, P, P, P, P, P]),
                            ("dpf_hip_dcf_expand_plan",
                             [I64, I, I, I, ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_lookup_supported", [P, I]),
                            ("dpf_hip_lookup_batch",
                             [I64, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, I, P, P]),
                            ("dpf_hip_lookup_plan",
                             [I64, I, I, I, ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_expand_rows_supported", [P]),
                            ("dpf_hip_expand_rows",
                             [I64, I, I, I, P, P, P, P, P, P, P, P, P, P, P, I64, P]),
                            ("dpf_hip_expand_rows_plan",
                             [I64, I, I, ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_dot_buckets",
                             [I64, I, I, ctypes.POINTER(ctypes.c_int64), I64, P, P, I64, P, P, P,
                              I64, P]),
                            ("dpf_hip_last_dot_buckets_shape", [ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_expand_sum_supported", [P]),
                            ("dpf_hip_expand_sum",
                             [I64, I, I, I, P, P, P, P, P, P, P, P, P, P, P, I64, P, I, P]),
                            ("dpf_hip_expand_sum_plan",
                             [I64, I, I, ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_expand_sum_packed_supported", [P]),
                            ("dpf_hip_expand_sum_packed",
                             [I64, I, I, I, P, P, P, P, P, P, P, P, P, P, P, I64, P, I64, I, P]),
                            ("dpf_hip_expand_sketch_supported", [P]),
                            ("dpf_hip_expand_sketch",
                             [I64, I, I, I, P, P, P, P, P, P, P, P, P, P, I, P, P, I64, P, P, I,
                              P]),
                            ("dpf_hip_expand_sketch_plan",
                             [I64, I, I, ctypes.POINTER(ctypes.c_int64)]),
                            ("dpf_hip_prefix_batch_max_expand", [P, I]),
                            ("dpf_hip_prefix_batch_level", [ctypes.POINTER(PrefixBatchArgs), P])):
            if hasattr(L, name):
                getattr(L, name).argtypes = types
        if hasattr(L, "dpf_hip_expand_sketch_workspace_bytes"):
            L.dpf_hip_expand_sketch_workspace_bytes.argtypes = [I64, I, I, I, I]
            L.dpf_hip_expand_sketch_workspace_bytes.restype = ctypes.c_int64
        if hasattr(L, "dpf_hip_expand_sum_workspace_bytes"):
            L.dpf_hip_expand_sum_workspace_bytes.argtypes = [I64, I]
            L.dpf_hip_expand_sum_workspace_bytes.restype = ctypes.c_int64
        if hasattr(L, "dpf_hip_dot_buckets_workspace_bytes"):
            L.dpf_hip_dot_buckets_workspace_bytes.argtypes = [P, I, I64, I64, I]
            L.dpf_hip_dot_buckets_workspace_bytes.restype = ctypes.c_int64
        if hasattr(L, "dpf_hip_last_dot_kernel"):
            L.dpf_hip_last_dot_kernel.restype = ctypes.c_char_p
        _lib = L
    if require_gpu:
        import torch
        if not torch.cuda.is_available():
            raise DpfHipError(13, "no GPU visible: the DPF engine has no CPU fallback")
    return _lib


def last_expand_kernel():
    """(kernel, subtree depth) of this thread's last dpf_hip_expand launch,
    e.g. ("octet/mod32", 3) -- dispatch diagnostics for the tests."""
    d = ctypes.c_int(-1)
    name = load().dpf_hip_last_expand_kernel(ctypes.byref(d)).decode()
    return name, d.value


def last_batch_kernel() -> str:
    """Kernel of this thread's last batched prefix evaluation, e.g. "hh_level"
    -- dispatch diagnostics for the tests."""
    return load().dpf_hip_last_batch_kernel().decode()


def last_points_kernel() -> str:
    """Kernel of this thread's last point evaluation, e.g. "points/ilp4" --
    dispatch diagnostics for the tests."""
    return load().dpf_hip_last_points_kernel().decode()


def last_dot_kernel() -> str:
    """Path of this thread's last dot call: "small", "pair" or "octet" (the
    fused expand kernel), "rows" (dot_rows), "select" (select_rows),
    "rows_batch" (dot_rows_batch) or "buckets" (dot_buckets) -- dispatch
    diagnostics for the tests."""
    return load().dpf_hip_last_dot_kernel().decode()


def dot_workspace_bytes(desc: ValueDesc, record_words: int) -> int:
    """Bytes of workspace expand_dot / dot_rows need (no GPU needed)."""
    n = load().dpf_hip_expand_dot_workspace_bytes(ctypes.byref(desc), record_words)
    if n < 0:
        raise DpfHipError(12 if 1 <= record_words <= 1024 else 3,
                          load().dpf_hip_last_error().decode())
    return n


def select_workspace_bytes(record_words: int, num_queries: int) -> int:
    """Bytes of workspace select_rows needs (no GPU needed)."""
    n = load().dpf_hip_select_workspace_bytes(record_words, num_queries)
    if n < 0:
        raise DpfHipError(3, load().dpf_hip_last_error().decode())
    return n


def last_select_shape():
    """(queries per tile, passes over the database, workgroups per pass) of
    this thread's last select_rows -- dispatch diagnostics for the tests."""
    a = (ctypes.c_int64 * 3)()
    check(load().dpf_hip_last_select_shape(a))
    return tuple(a)


def dot_batch_workspace_bytes(desc: ValueDesc, record_words: int, num_queries: int) -> int:
    """Bytes of workspace dot_rows_batch needs (no GPU needed)."""
    n = load().dpf_hip_dot_rows_batch_workspace_bytes(ctypes.byref(desc), record_words,
                                                      num_queries)
    if n < 0:
        raise DpfHipError(12 if 1 <= record_words <= 1024 and 1 <= num_queries <= 64 else 3,
                          load().dpf_hip_last_error().decode())
    return n


def last_dot_batch_shape():
    """(queries per tile, passes over the database, workgroups per pass) of
    this thread's last dot_rows_batch -- dispatch diagnostics for the tests."""
    a = (ctypes.c_int64 * 3)()
    check(load().dpf_hip_last_dot_batch_shape(a))
    return tuple(a)


def last_dynamic_chunks() -> int:
    """Chunks of 64 items per workgroup of this thread's last launch that can
    take its work dynamically (0: the fixed grid-stride share) -- schedule
    diagnostics for the tests."""
    n = ctypes.c_int64(-1)
    check(load().dpf_hip_last_dynamic_chunks(ctypes.byref(n)))
    return n.value


def dcf_expand_plan(num_keys: int, num_levels: int, shard_bits: int, compute_units: int) -> dict:
    """The launch plan of dpf_hip_dcf_expand for that shape (no GPU needed):
    {"G", "walk", "items", "items_per_key", "top_G", "top_items"}; top_G is
    -1 when no first launch leaves the items their roots."""
    out = (ctypes.c_int64 * 6)()
    check(load().dpf_hip_dcf_expand_plan(num_keys, num_levels, shard_bits, compute_units, out))
    return {"G": out[0], "walk": out[1], "items": out[2], "items_per_key": out[3],
            "top_G": out[4], "top_items": out[5]}


def lookup_plan(num_keys: int, tree_depth: int, table_words: int, compute_units: int) -> dict:
    """The launch plan of dpf_hip_lookup_batch for that shape (no GPU needed):
    {"S", "walk", "items_per_key", "items"}."""
    out = (ctypes.c_int64 * 4)()
    check(load().dpf_hip_lookup_plan(num_keys, tree_depth, table_words, compute_units, out))
    return {"S": out[0], "walk": out[1], "items_per_key": out[2], "items": out[3]}


def lookup_supported(desc, table_words: int) -> bool:
    """Whether dpf_hip_lookup_batch takes this value type and table width
    (`desc` None: a NULL descriptor; no GPU needed)."""
    return bool(load().dpf_hip_lookup_supported(ctypes.byref(desc) if desc is not None else None,
                                                table_words))


EXPAND_ROWS_MAX_SUBTREE = 6   # DPF_HIP_EXPAND_ROWS_MAX_SUBTREE


def expand_rows_plan(num_keys: int, tree_depth: int, compute_units: int) -> dict:
    """The launch plan of dpf_hip_expand_rows for that shape (no GPU needed):
    {"S", "walk", "items_per_key", "items"}."""
    out = (ctypes.c_int64 * 4)()
    check(load().dpf_hip_expand_rows_plan(num_keys, tree_depth, compute_units, out))
    return {"S": out[0], "walk": out[1], "items_per_key": out[2], "items": out[3]}


def expand_rows_supported(desc) -> bool:
    """Whether dpf_hip_expand_rows and dpf_hip_dot_buckets take this value type
    (`desc` None: a NULL descriptor; no GPU needed)."""
    return bool(load().dpf_hip_expand_rows_supported(
        ctypes.byref(desc) if desc is not None else None))


def dot_buckets_workspace_bytes(desc, record_words: int, num_buckets: int, num_keys: int,
                                log_domain_size: int) -> int:
    """Bytes of dpf_hip_dot_buckets' workspace for those counts (no GPU
    needed); -1 for arguments out of range or a value type it does not take."""
    return int(load().dpf_hip_dot_buckets_workspace_bytes(
        ctypes.byref(desc) if desc is not None else None, record_words, num_buckets, num_keys,
        log_domain_size))


def last_dot_buckets_shape():
    """(work items, tiles, largest tile, column chunks) of this thread's last
    dot_buckets that launched -- dispatch diagnostics for the tests."""
    a = (ctypes.c_int64 * 4)()
    check(load().dpf_hip_last_dot_buckets_shape(a))
    return tuple(a)


EXPAND_SUM_WAVE_ITEMS_PER_CU = 64   # DPF_HIP_EXPAND_SUM_WAVE_ITEMS_PER_CU


def expand_sum_plan(num_keys: int, tree_depth: int, compute_units: int) -> dict:
    """The launch plan of dpf_hip_expand_sum for that shape (no GPU needed):
    {"S", "walk", "subtrees", "wave_items", "group", "threshold"}."""
    out = (ctypes.c_int64 * 6)()
    check(load().dpf_hip_expand_sum_plan(num_keys, tree_depth, compute_units, out))
    return {"S": out[0], "walk": out[1], "subtrees": out[2], "wave_items": out[3],
            "group": out[4], "threshold": out[5]}


def expand_sum_supported(desc) -> bool:
    """Whether dpf_hip_expand_sum takes this value type (`desc` None: a NULL
    descriptor; no GPU needed)."""
    return bool(load().dpf_hip_expand_sum_supported(
        ctypes.byref(desc) if desc is not None else None))


def expand_sum_packed_supported(desc) -> bool:
    """Whether dpf_hip_expand_sum_packed takes this value type (`desc` None: a
    NULL descriptor; no GPU needed)."""
    return bool(load().dpf_hip_expand_sum_packed_supported(
        ctypes.byref(desc) if desc is not None else None))


def expand_sum_workspace_bytes(num_keys: int, num_levels: int) -> int:
    """Bytes of dpf_hip_expand_sum's workspace for that batch (no GPU needed);
    -1 for arguments out of range."""
    return int(load().dpf_hip_expand_sum_workspace_bytes(num_keys, num_levels))


EXPAND_SKETCH_WAVE_ITEMS_PER_CU = 64   # DPF_HIP_EXPAND_SKETCH_WAVE_ITEMS_PER_CU
EXPAND_SKETCH_MAX_LOG_DOMAIN = 28      # DPF_HIP_EXPAND_SKETCH_MAX_LOG_DOMAIN


def expand_sketch_plan(num_keys: int, tree_depth: int, compute_units: int) -> dict:
    """The launch plan of dpf_hip_expand_sketch for that shape (no GPU needed;
    DPF_EXPAND_SKETCH_WAVE_ITEMS in the environment replaces the threshold):
    {"S", "walk", "subtrees", "wave_items", "group", "threshold"}."""
    out = (ctypes.c_int64 * 6)()
    check(load().dpf_hip_expand_sketch_plan(num_keys, tree_depth, compute_units, out))
    return {"S": out[0], "walk": out[1], "subtrees": out[2], "wave_items": out[3],
            "group": out[4], "threshold": out[5]}


def expand_sketch_supported(desc) -> bool:
    """Whether dpf_hip_expand_sketch takes this value type (`desc` None: a NULL
    descriptor; no GPU needed)."""
    return bool(load().dpf_hip_expand_sketch_supported(
        ctypes.byref(desc) if desc is not None else None))


def expand_sketch_workspace_bytes(num_keys: int, num_levels: int, log_domain_size: int,
                                  num_leaves: int, num_weights: int) -> int:
    """Bytes of dpf_hip_expand_sketch's workspace for that call (no GPU needed);
    -1 for arguments out of range."""
    return int(load().dpf_hip_expand_sketch_workspace_bytes(
        num_keys, num_levels, log_domain_size, num_leaves, num_weights))


def clock_probe(on: bool) -> None:
    """Turns the expand launches' in-kernel clock probe on (zeroed) or off."""
    check(load(require_gpu=True).dpf_hip_clock_probe(1 if on else 0))


def clock_probe_read() -> dict:
    """Sustained shader clock (GHz) of the octet expand launches since the
    last read, from s_memtime / s_memrealtime stamps of every workgroup."""
    ghz, wg, mean_s = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    check(load().dpf_hip_clock_probe_read(ctypes.byref(ghz), ctypes.byref(wg), ctypes.byref(mean_s)))
    return {"clock_ghz": ghz.value, "workgroups": wg.value, "mean_workgroup_ms": mean_s.value * 1e3}


def clock_probe_exits() -> dict:
    """When the waves of the last expand launch left the kernel, in ms after
    its first workgroup began (call after one launch, before
    clock_probe_read, which zeroes the stamps)."""
    out = (ctypes.c_double * 6)()
    check(load().dpf_hip_clock_probe_exits(out))
    ms = [v * 1e3 for v in out[:5]]
    return {"first_exit_ms": ms[0], "last_exit_ms": ms[1], "workgroup_last_exit_min_ms": ms[2],
            "workgroup_last_exit_max_ms": ms[3], "workgroup_last_exit_mean_ms": ms[4],
            "workgroups": int(out[5])}


def octet_schedule(num_items: int, k0: int, subtree_depth: int, min_depth: int,
                   compute_units: int) -> dict:
    """The chunk schedule of a full-domain expand launch of that shape (no
    GPU needed; reads the DPF_OCTET_* hooks): {"shift", "global", "counters",
    "phases": [{"chunks", "first_item", "k0", "depth"}]}, phases in the order
    they are taken; shift 0 is a static launch without phases."""
    out = (ctypes.c_int64 * 15)()
    check(load().dpf_hip_octet_schedule(num_items, k0, subtree_depth, min_depth, compute_units,
                                        out))
    return _plan(out)


def last_expand_schedule() -> dict:
    """The chunk schedule this thread's last expand launch ran with on its
    device, as octet_schedule returns it (shift 0: a static launch)."""
    out = (ctypes.c_int64 * 15)()
    check(load().dpf_hip_last_expand_schedule(out))
    return _plan(out)


def _plan(out) -> dict:
    phases = [{"chunks": out[3 + 4 * j], "first_item": out[4 + 4 * j], "k0": out[5 + 4 * j],
               "depth": out[6 + 4 * j]} for j in range(3) if out[3 + 4 * j]]
    return {"shift": out[0], "global": bool(out[1]), "counters": out[2], "phases": phases}


def check(st: int):
    if st != 0:
        raise DpfHipError(st, load().dpf_hip_last_error().decode())


def aes_key(k: int) -> AesKey:
    a = AesKey()
    for i, b in enumerate((k & ((1 << 128) - 1)).to_bytes(16, "little")):
        a.bytes[i] = b
    return a


def value_desc(leaves: Sequence[tuple], direct: bool, elements_per_block: int,
               blocks_needed: int) -> ValueDesc:
    """leaves: [(kind, bits, modulus)]."""
    d = ValueDesc()
    d.num_leaves = len(leaves)
    d.direct = 1 if direct else 0
    d.elements_per_block = elements_per_block
    d.blocks_needed = blocks_needed
    for i, (kind, bits, mod) in enumerate(leaves):
        d.kind[i] = kind
        d.bits[i] = bits
        d.mod_low[i] = mod & MASK64
        d.mod_high[i] = (mod >> 64) & MASK64
    return d


def _p(t) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def _stream(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def to_device_blocks(a: np.ndarray, device="cuda"):
    """numpy uint64 (n, 2) -> torch int64 tensor (n, 2) on device (same bytes)."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 2)
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_device_u8(a, device="cuda"):
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return torch.from_numpy(a).to(device)


def blocks_to_numpy(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64).reshape(-1, 2)


def hash_blocks(blocks, key: int, out=None, stream=None):
    import torch
    L = load(require_gpu=True)
    n = blocks.shape[0]
    if out is None:
        out = torch.empty_like(blocks)
    k = aes_key(key)
    check(L.dpf_hip_hash(n, _p(blocks), ctypes.byref(k), _p(out), _stream(stream)))
    return out


def eval_paths(seeds, ctrl, paths, cw_seed, cw_left, cw_right, key_left: int, key_right: int,
               seeds_out=None, ctrl_out=None, stream=None):
    import torch
    L = load(require_gpu=True)
    n = seeds.shape[0]
    levels = cw_left.shape[0]
    if seeds_out is None:
        seeds_out = torch.empty_like(seeds)
    if ctrl_out is None:
        ctrl_out = torch.empty_like(ctrl)
    kl, kr = aes_key(key_left), aes_key(key_right)
    check(L.dpf_hip_eval_paths(n, levels, _p(seeds), _p(ctrl), _p(paths), _p(cw_seed),
                               _p(cw_left), _p(cw_right), ctypes.byref(kl), ctypes.byref(kr),
                               _p(seeds_out), _p(ctrl_out), _stream(stream)))
    return seeds_out, ctrl_out


def expand(seeds, ctrl, cw_seed, cw_left, cw_right, keys, desc: ValueDesc, elements_per_leaf: int,
           value_correction, party: int, out=None, stream=None):
    """Fused ExpandSeeds + HashExpandedSeeds + correction; returns packed uint8 tensor."""
    import torch
    L = load(require_gpu=True)
    n0 = seeds.shape[0]
    levels = cw_left.shape[0]
    esz = L.dpf_hip_packed_element_size(ctypes.byref(desc))
    total = (n0 << levels) * elements_per_leaf
    if out is None:
        out = torch.empty(total * esz, dtype=torch.uint8, device=seeds.device)
    kl, kr, kv = (aes_key(k) for k in keys)
    check(L.dpf_hip_expand(n0, _p(seeds), _p(ctrl), levels, _p(cw_seed), _p(cw_left),
                           _p(cw_right), ctypes.byref(kl), ctypes.byref(kr), ctypes.byref(kv),
                           ctypes.byref(desc), elements_per_leaf, _p(value_correction), party,
                           _p(out), _stream(stream)))
    return out


def _dot_buffers(desc, record_words, workspace, out, device):
    import torch
    esz = load().dpf_hip_packed_element_size(ctypes.byref(desc))
    if workspace is None:
        workspace = torch.empty(dot_workspace_bytes(desc, record_words), dtype=torch.uint8,
                                device=device)
    if out is None:
        out = torch.empty(record_words * esz, dtype=torch.uint8, device=device)
    return workspace, out


def expand_dot(seeds, ctrl, cw_seed, cw_left, cw_right, keys, desc: ValueDesc,
               elements_per_leaf: int, value_correction, party: int, db, record_words: int = 1,
               workspace=None, out=None, stream=None):
    """expand() folded into the database `db` at the leaves (no share vector
    is stored); returns `record_words` packed elements as a uint8 tensor."""
    L = load(require_gpu=True)
    workspace, out = _dot_buffers(desc, record_words, workspace, out, seeds.device)
    kl, kr, kv = (aes_key(k) for k in keys)
    check(L.dpf_hip_expand_dot(seeds.shape[0], _p(seeds), _p(ctrl), cw_left.shape[0], _p(cw_seed),
                               _p(cw_left), _p(cw_right), ctypes.byref(kl), ctypes.byref(kr),
                               ctypes.byref(kv), ctypes.byref(desc), elements_per_leaf,
                               _p(value_correction), party, _p(db), record_words, _p(workspace),
                               _p(out), _stream(stream)))
    return out


def dot_rows(num_rows: int, record_words: int, desc: ValueDesc, y, db, accumulate: bool = False,
             workspace=None, out=None, stream=None):
    """out[w] (+)= fold of the packed share vector `y` into `db`'s first
    num_rows records; returns `record_words` packed elements (uint8 tensor)."""
    L = load(require_gpu=True)
    workspace, out = _dot_buffers(desc, record_words, workspace, out, db.device)
    check(L.dpf_hip_dot_rows(num_rows, record_words, ctypes.byref(desc), _p(y), _p(db),
                             1 if accumulate else 0, _p(workspace), _p(out), _stream(stream)))
    return out


def select_rows(num_rows: int, record_words: int, num_queries: int, sel, sel_stride_bytes: int,
                db, accumulate: bool = False, workspace=None, out=None, stream=None):
    """out[q][w] (^)= XOR of db[j][w] over the rows j < num_rows whose bit j of
    row q of `sel` (device bytes, rows sel_stride_bytes apart) is set; returns
    (num_queries, record_words) as an int64 tensor (the bits of uint64)."""
    import torch
    L = load(require_gpu=True)
    if workspace is None:
        workspace = torch.empty(select_workspace_bytes(record_words, num_queries),
                                dtype=torch.uint8, device=db.device)
    if out is None:
        out = torch.empty((num_queries, record_words), dtype=torch.int64, device=db.device)
    check(L.dpf_hip_select_rows(num_rows, record_words, num_queries, _p(sel), sel_stride_bytes,
                                _p(db), 1 if accumulate else 0, _p(workspace), _p(out),
                                _stream(stream)))
    return out


def dot_rows_batch(num_rows: int, record_words: int, num_queries: int, desc: ValueDesc, y,
                   y_stride_bytes: int, db, accumulate: bool = False, workspace=None, out=None,
                   stream=None):
    """out[q][w] (+)= fold of row q of `y` (device, packed 8-byte shares, rows
    y_stride_bytes apart) into `db`'s first num_rows records: sums mod 2^64 for
    uint64, XOR of ANDs for XorWrapper<uint64>; returns (num_queries,
    record_words) as an int64 tensor (the bits of uint64)."""
    import torch
    L = load(require_gpu=True)
    if workspace is None:
        workspace = torch.empty(dot_batch_workspace_bytes(desc, record_words, num_queries),
                                dtype=torch.uint8, device=db.device)
    if out is None:
        out = torch.empty((num_queries, record_words), dtype=torch.int64, device=db.device)
    check(L.dpf_hip_dot_rows_batch(num_rows, record_words, num_queries, ctypes.byref(desc), _p(y),
                                   y_stride_bytes, _p(db), 1 if accumulate else 0, _p(workspace),
                                   _p(out), _stream(stream)))
    return out


def expand_rows(log_domain_size: int, key_seed, party, cw_seed, cw_left, cw_right, keys,
                desc: ValueDesc, value_correction, rows=None, row_stride_bytes=None,
                cw_stride=None, stream=None):
    """dpf_hip_expand_rows on torch device tensors: key_seed (K, 2) int64, party
    (K,) uint8, cw_seed (K, cw_stride, 2) int64, cw_left / cw_right (K,
    cw_stride) uint8, value_correction (2 K, 2) int64, keys = (left, right,
    value) AES keys as integers.  Returns `rows`: K rows of row_stride_bytes /
    8 int64 (the bits of uint64; default stride 8 * 2^n), of which the first
    2^n of every row are written."""
    import torch
    L = load(require_gpu=True)
    K, n = int(key_seed.shape[0]), int(log_domain_size)
    stride = (8 << n) if row_stride_bytes is None else int(row_stride_bytes)
    if cw_stride is None:
        cw_stride = n - 1
    if rows is None:
        rows = torch.empty((max(K, 1), stride // 8), dtype=torch.int64, device=key_seed.device)
    kl, kr, kv = (aes_key(k) for k in keys)
    check(L.dpf_hip_expand_rows(K, n - 1, int(cw_stride), n, _p(key_seed), _p(party), _p(cw_seed),
                                _p(cw_left), _p(cw_right), ctypes.byref(kl), ctypes.byref(kr),
                                ctypes.byref(kv), ctypes.byref(desc), _p(value_correction),
                                _p(rows), stride, _stream(stream)))
    return rows


def dot_buckets(log_domain_size: int, record_words: int, bucket_begin, desc: ValueDesc, y,
                y_stride_bytes: int, db, out=None, workspace=None, stream=None):
    """out[k][w] = fold of row k of `y` (device, 8-byte shares, rows
    y_stride_bytes apart) into the slice db[b(k)] of `db` (device, [B][2^n]
    [record_words] uint64), b(k) given by the B + 1 host integers
    `bucket_begin`: sums mod 2^64 for uint64, XOR of ANDs for
    XorWrapper<uint64>; returns (K, record_words) as an int64 tensor (the bits
    of uint64).  The workspace is a fresh tensor unless given."""
    import torch
    L = load(require_gpu=True)
    bb = (ctypes.c_int64 * len(bucket_begin))(*[int(x) for x in bucket_begin])
    B, K = len(bucket_begin) - 1, int(bucket_begin[-1])
    if workspace is None:
        need = dot_buckets_workspace_bytes(desc, record_words, B, K, log_domain_size)
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=db.device)
    if out is None:
        out = torch.empty((K, record_words), dtype=torch.int64, device=db.device)
    check(L.dpf_hip_dot_buckets(B, log_domain_size, record_words, bb, K, ctypes.byref(desc),
                                _p(y), y_stride_bytes, _p(db), _p(out), _p(workspace),
                                workspace.numel(), _stream(stream)))
    return out


def sketch_rows(num_keys: int, row_len: int, desc: ValueDesc, rows, weights, out=None,
                weight_bits: int = 32, stream=None):
    """out[k][j][e] = (sum_i (weights[j][i] mod N_e) * rows[k][i][e]) mod N_e for
    `rows` = num_keys rows of row_len packed elements of a tuple of
    IntModN<uint32> (device bytes) and `weights` (J, row_len) 32-bit; returns
    (num_keys, J, num_leaves) as an int32 tensor (the bits of uint32)."""
    import torch
    L = load(require_gpu=True)
    J = int(weights.shape[0])
    if out is None:
        out = torch.empty((num_keys, J, desc.num_leaves), dtype=torch.int32, device=rows.device)
    check(L.dpf_hip_sketch_rows(num_keys, row_len, ctypes.byref(desc), _p(rows), J, weight_bits,
                                _p(weights), _p(out), _stream(stream)))
    return out


def expand_sketch(log_domain_size: int, key_seed, party, cw_seed, cw_left, cw_right, keys,
                  desc: ValueDesc, value_correction, weights=None, sum_out=None,
                  accumulate: bool = False, workspace=None, stream=None):
    """dpf_hip_expand_sketch on torch device tensors: key_seed (K, 2) int64,
    party (K,) uint8, cw_seed (K, n, 2) int64, cw_left / cw_right (K, n) uint8,
    value_correction (K * nl, 2) int64, weights (J, 2^n) int32 or None, keys =
    (left, right, value) AES keys as integers.  Returns (sums int32 [2^n, nl],
    sketches int32 [K, J, nl]); the workspace is a fresh tensor unless given."""
    import torch
    L = load(require_gpu=True)
    K, n, nl = int(key_seed.shape[0]), int(log_domain_size), int(desc.num_leaves)
    J = 0 if weights is None else int(weights.shape[0])
    need = expand_sketch_workspace_bytes(K, n, n, nl, J)
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=key_seed.device)
    if sum_out is None:
        make = torch.zeros if accumulate else torch.empty
        sum_out = make((1 << n, nl), dtype=torch.int32, device=key_seed.device)
    sketch = torch.empty((K, J, nl), dtype=torch.int32, device=key_seed.device)
    kl, kr, kv = (aes_key(k) for k in keys)
    check(L.dpf_hip_expand_sketch(K, n, n, n, _p(key_seed), _p(party), _p(cw_seed), _p(cw_left),
                                  _p(cw_right), ctypes.byref(kl), ctypes.byref(kr),
                                  ctypes.byref(kv), ctypes.byref(desc), _p(value_correction), J,
                                  _p(weights), _p(workspace), workspace.numel(), _p(sum_out),
                                  _p(sketch) if J else None, 1 if accumulate else 0,
                                  _stream(stream)))
    return sum_out, sketch


def eval_points(n, points_per_key, levels, key_seed, party, tree_index, block_index, cw_seed,
                cw_left, cw_right, keys, desc: ValueDesc, value_correction, seeds_in=None,
                ctrl_in=None, out=None, stream=None):
    import torch
    L = load(require_gpu=True)
    esz = L.dpf_hip_packed_element_size(ctypes.byref(desc))
    if out is None:
        out = torch.empty(max(n * esz, 1), dtype=torch.uint8, device=tree_index.device)
    kl, kr, kv = (aes_key(k) for k in keys)
    check(L.dpf_hip_eval_points(n, points_per_key, levels, _p(key_seed), _p(party), _p(seeds_in),
                                _p(ctrl_in), _p(tree_index), _p(block_index), _p(cw_seed),
                                _p(cw_left), _p(cw_right), ctypes.byref(kl), ctypes.byref(kr),
                                ctypes.byref(kv), ctypes.byref(desc), _p(value_correction),
                                _p(out), _stream(stream)))
    return out


def gen_key_batch(num_keys: int, num_levels: int, tree_level: Sequence[int],
                  log_domain: Sequence[int], blocks: Sequence[int], descs: Sequence[ValueDesc],
                  alphas, root_seeds, beta, beta_mode: int, dcf_bits: int, keys, cw_seed, cw_left,
                  cw_right, value_correction: Sequence, stream=None) -> None:
    """Both parties' correction words of num_keys key pairs into caller-owned
    device buffers: `tree_level`, `log_domain`, `blocks` and `descs` hold one
    entry per hierarchy level; `alphas` (num_keys blocks), `root_seeds`
    ([key][party] blocks) and `beta` (blocks: per level, per key and level, or
    per key for beta_mode 0, 1, 2) are device tensors; `cw_seed` (num_keys *
    num_levels blocks), `cw_left` / `cw_right` (as many bytes, any alignment)
    and value_correction[h] (num_keys * elements per block blocks) are written."""
    L = load(require_gpu=True)
    H = len(descs)
    if not (len(tree_level) == len(log_domain) == len(blocks) == len(value_correction) == H):
        raise DpfHipError(3, "gen_key_batch: one table entry per hierarchy level")
    I32 = ctypes.c_int32 * H
    desc = (ValueDesc * H)(*descs)
    vc = (ctypes.c_void_p * H)(*[_p(t) for t in value_correction])
    kl, kr, kv = (aes_key(k) for k in keys)
    check(L.dpf_hip_gen_key_batch(num_keys, num_levels, H, I32(*tree_level), I32(*log_domain),
                                  I32(*blocks), desc, _p(alphas), _p(root_seeds), _p(beta),
                                  beta_mode, dcf_bits, ctypes.byref(kl), ctypes.byref(kr),
                                  ctypes.byref(kv), _p(cw_seed), _p(cw_left), _p(cw_right), vc,
                                  _stream(stream)))


class Event:
    """hipEvent on an explicit stream (torch.cuda.Event only sees torch's stream)."""

    def __init__(self):
        self.ev = ctypes.c_void_p()
        check(load().dpf_hip_event_create(ctypes.byref(self.ev)))

    def record(self, stream=None):
        check(load().dpf_hip_event_record(self.ev, _stream(stream)))

    def elapsed_ms(self, end: "Event") -> float:
        ms = ctypes.c_float()
        check(load().dpf_hip_event_elapsed_ms(self.ev, end.ev, ctypes.byref(ms)))
        return float(ms.value)

    def __del__(self):
        try:
            if _lib is not None and self.ev:
                _lib.dpf_hip_event_destroy(self.ev)
        except Exception:
            pass
