"""CPU checks of the C-ABI library: it loads and exports every symbol that
include/dpf_hip.h declares (no compute calls without a GPU)."""
import ctypes

from distributed_point_functions_amd import hip_abi


def test_header_declares_hot_path_entry_points():
    fns = hip_abi.header_functions()
    for f in ("dpf_hip_hash", "dpf_hip_eval_paths", "dpf_hip_expand", "dpf_hip_eval_points"):
        assert f in fns


def test_library_exports_every_declared_symbol():
    lib = hip_abi.load()
    missing = [f for f in hip_abi.header_functions() if not hasattr(lib, f)]
    assert missing == []


def test_abi_version_and_packed_size():
    lib = hip_abi.load()
    assert lib.dpf_hip_abi_version() == 2
    d = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0), (hip_abi.LEAF_INT, 64, 0)], True, 1, 1)
    assert lib.dpf_hip_packed_element_size(ctypes.byref(d)) == 12


def test_argument_validation_without_gpu():
    # Validation happens before any device work, so it is testable on CPU.
    lib = hip_abi.load()
    d = hip_abi.value_desc([(hip_abi.LEAF_INT, 4, 0)], True, 32, 1)
    k = hip_abi.aes_key(0)
    st = lib.dpf_hip_expand(1, None, None, 3, None, None, None, ctypes.byref(k), ctypes.byref(k),
                            ctypes.byref(k), ctypes.byref(d), 1, None, 0, None, None)
    assert st == 12  # UNIMPLEMENTED: 4-bit leaves have no C++ type in the reference
    assert b"power of two" in lib.dpf_hip_last_error()
    st = lib.dpf_hip_hash(-1, None, ctypes.byref(k), None, None)
    assert st == 3


def _empty_batch(desc, **members):
    """A launch description with no keys and no start nodes: every check of
    dpf_hip_prefix_batch_level that reads no device memory runs, nothing is
    launched and no device is touched."""
    return hip_abi.prefix_batch_args(**{"desc": ctypes.pointer(desc), "cw_stride": 1,
                                        "elements_per_leaf": 1, **members})


def _u64():
    return hip_abi.value_desc([(hip_abi.LEAF_INT, 64, 0)], True, 2, 1)


def test_prefix_batch_args_size_handshake():
    lib = hip_abi.load()
    a = _empty_batch(_u64())
    assert a.struct_size == ctypes.sizeof(hip_abi.PrefixBatchArgs)
    assert lib.dpf_hip_prefix_batch_level(ctypes.byref(a), None) == 0
    a.struct_size -= 1
    assert lib.dpf_hip_prefix_batch_level(ctypes.byref(a), None) == 3
    assert b"dpf_prefix_batch_args" in lib.dpf_hip_last_error()
    assert lib.dpf_hip_prefix_batch_level(None, None) == 3
    assert b"dpf_prefix_batch_args" in lib.dpf_hip_last_error()


def test_prefix_batch_args_fields_land_where_the_library_reads_them():
    """The ctypes mirror and the C struct agree on the integer members: each
    one, set alone, trips the check that reads it."""
    lib = hip_abi.load()
    mixed = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0), (hip_abi.LEAF_INT, 64, 0)], True, 1, 1)
    assert lib.dpf_hip_prefix_batch_max_expand(ctypes.byref(mixed), 1) < 0
    nibble = hip_abi.value_desc([(hip_abi.LEAF_INT, 4, 0)], True, 32, 1)
    for desc, members, code, msg in (
            (_u64(), {"elements_per_leaf": 0}, 3, b"elements_per_leaf must be in"),
            (_u64(), {"expand_levels": 99}, 3, b"level arguments out of range"),
            (_u64(), {"cw_first": 1, "cw_stride": 1, "walk_levels": 1}, 3,
             b"level arguments out of range"),
            (nibble, {}, 12, b"power of two"),
            (mixed, {"sum": 1}, 12, b"no on-device key sum")):
        a = _empty_batch(desc, **members)
        assert lib.dpf_hip_prefix_batch_level(ctypes.byref(a), None) == code, members
        assert msg in lib.dpf_hip_last_error(), members


def test_prefix_batch_fused_sketch_preconditions_without_gpu():
    lib = hip_abi.load()
    desc = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 32, 4294967291)], False, 1, 1)
    shape = {"expand_levels": 2, "cw_stride": 2, "sum": 1, "index_major": 1, "seeds_in": 16}
    assert lib.dpf_hip_prefix_batch_sketch_fused(ctypes.byref(desc), 0, 2, 1, 1, 1, 2) == 1
    a = _empty_batch(desc, num_weights=3, **shape)   # above kHHSketchMaxRows
    assert lib.dpf_hip_prefix_batch_level(ctypes.byref(a), None) == 12
    assert b"no fused sketch for this launch" in lib.dpf_hip_last_error()
