"""Full-domain DCF evaluation (dpf_hip_dcf_expand, EvaluateFullDomain*,
EvaluateRangeDot*) as far as it can be checked without a GPU: the C ABI's
declarations, the supported types, the argument checks, the launch plan and the
order of the host API's checks."""
import ctypes
import re

import pytest
import torch

from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from test_dcf_cpu import make

INVALID_ARGUMENT, UNIMPLEMENTED = 3, 12
K_G_MAX = 11   # kGMax (dpf_device.h)
SYMBOLS = ("dpf_hip_dcf_expand", "dpf_hip_dcf_expand_supported", "dpf_hip_dcf_expand_plan")


class _NullStream:
    cuda_stream = 0


class _Buffer:
    """Stands in for a device tensor: an address and a size, never read."""

    def __init__(self, ptr, nbytes, device="cpu"):
        self._ptr, self._n, self.device = ptr, nbytes, device

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n

    def element_size(self):
        return 1


def _desc(kind, bits):
    return hip_abi.value_desc([(kind, bits, 0)], True, 128 // bits, 1)


def test_header_and_abi_declare_the_entry_points():
    names = hip_abi.header_functions()
    lib = hip_abi.load()
    src = open(hip_abi.__file__).read()
    for f in SYMBOLS:
        assert f in names
        assert hasattr(lib, f), f
        assert re.search(r'"%s",' % f, src), f
        assert getattr(lib, f).argtypes is not None
    assert lib.dpf_hip_abi_version() == 2


@pytest.mark.parametrize("kind", [hip_abi.LEAF_INT, hip_abi.LEAF_XOR])
@pytest.mark.parametrize("bits", [8, 16, 32, 64, 128])
def test_supported_types(kind, bits):
    lib = hip_abi.load()
    n = 9
    depth = (ctypes.c_int32 * n)(*range(n))
    assert lib.dpf_hip_dcf_expand_supported(ctypes.byref(_desc(kind, bits)), n, depth) == 1


def test_unsupported_types_hierarchies_and_null():
    lib = hip_abi.load()
    n = 9
    depth = (ctypes.c_int32 * n)(*range(n))
    ok = _desc(hip_abi.LEAF_INT, 64)
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, 18446744073709551557)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    for d in (modn, pair):
        assert lib.dpf_hip_dcf_expand_supported(ctypes.byref(d), n, depth) == 0
    flat = (ctypes.c_int32 * n)(0, 1, 2, 3, 3, 4, 5, 6, 7)      # a level that shares a depth
    assert lib.dpf_hip_dcf_expand_supported(ctypes.byref(ok), n, flat) == 0
    assert lib.dpf_hip_dcf_expand_supported(None, n, depth) == 0
    assert lib.dpf_hip_dcf_expand_supported(ctypes.byref(ok), n, None) == 0
    assert lib.dpf_hip_dcf_expand_supported(ctypes.byref(ok), 0, depth) == 0


def _abi_args(desc=None, **over):
    """A call of dpf_hip_dcf_expand whose pointers are non-null dummies: it
    must be rejected before anything dereferences them."""
    blocks = (ctypes.c_uint64 * 64)()
    ptrs = (ctypes.c_void_p * 128)(*([ctypes.addressof(blocks)] * 128))
    p = ctypes.cast(blocks, ctypes.c_void_p)
    key = hip_abi.aes_key(0)
    kp = ctypes.cast(ctypes.pointer(key), ctypes.c_void_p)
    d = desc if desc is not None else _desc(hip_abi.LEAF_INT, 64)
    a = dict(num_keys=2, n=8, shard_bits=0, shard_index=0, key_seed=p, party=p, cw_seed=p,
             cw_left=p, cw_right=p, cw_stride=7, vcw=ctypes.cast(ptrs, ctypes.c_void_p), kl=kp,
             kr=kp, kv=kp, desc=ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), out=p,
             stream=None)
    a.update(over)
    return list(a.values()), (blocks, ptrs, key, d)


@pytest.mark.parametrize("over", [
    dict(num_keys=-1), dict(n=0), dict(n=-3), dict(n=129),
    dict(shard_bits=-1), dict(shard_bits=8), dict(shard_bits=9),
    dict(shard_bits=3, shard_index=8), dict(shard_bits=3, shard_index=-1), dict(shard_index=1),
    dict(n=64), dict(n=70, shard_bits=7, cw_stride=69),
    dict(vcw=None), dict(kl=None), dict(kr=None), dict(kv=None),
    dict(key_seed=None), dict(party=None), dict(cw_seed=None), dict(cw_left=None),
    dict(cw_right=None), dict(out=None), dict(cw_stride=6),
], ids=str)
def test_argument_errors_are_invalid_argument(over):
    lib = hip_abi.load()
    args, keep = _abi_args(**over)
    assert lib.dpf_hip_dcf_expand(*args) == INVALID_ARGUMENT
    assert lib.dpf_hip_last_error()


def test_null_value_correction_of_one_level():
    lib = hip_abi.load()
    args, keep = _abi_args()
    keep[1][5] = None
    assert lib.dpf_hip_dcf_expand(*args) == INVALID_ARGUMENT
    assert b"NULL value correction" in lib.dpf_hip_last_error()


def test_unsupported_type_is_unimplemented_and_empty_call_is_ok():
    lib = hip_abi.load()
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, 18446744073709551557)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    for d in (modn, pair):
        args, keep = _abi_args(desc=d)
        assert lib.dpf_hip_dcf_expand(*args) == UNIMPLEMENTED
    args, keep = _abi_args(desc=None)
    args[14] = None     # a NULL descriptor
    assert lib.dpf_hip_dcf_expand(*args) == UNIMPLEMENTED
    # Nothing to do: OK without touching a device, even with null arrays.
    args, keep = _abi_args(num_keys=0, key_seed=None, party=None, out=None)
    assert lib.dpf_hip_dcf_expand(*args) == 0


@pytest.mark.parametrize("num_cus", [1, 256])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 13, 20, 30])
@pytest.mark.parametrize("num_keys", [1, 3, 37, 4096])
def test_plan_properties(num_keys, n, num_cus):
    for sb in sorted({0, min(1, n - 1), n - 1}):
        pl = hip_abi.dcf_expand_plan(num_keys, n, sb, num_cus)
        G, walk = pl["G"], pl["walk"]
        assert pl["items"] * 2 ** (G + 1) == num_keys * 2 ** (n - sb), (sb, pl)
        assert 0 <= G <= K_G_MAX
        assert walk + G == n - 1
        assert pl["items"] == num_keys * pl["items_per_key"]
        # An item deeper than one node belongs to a wave of items of its key.
        assert G == 0 or pl["items_per_key"] % 64 == 0
        if pl["top_G"] >= 0:
            # The stored root fits the item's outputs whatever the width, the
            # top items lie below the shard's root and fill waves per key.
            assert 2 ** (G + 1) >= 32
            top_root = walk - pl["top_G"] - 1
            assert top_root >= sb and (top_root - sb) >= 6
            assert pl["top_items"] * 2 ** (pl["top_G"] + 1) == pl["items"]
        else:
            assert pl["top_G"] == -1 and pl["top_items"] == 0


def test_plan_takes_both_paths_and_rejects_bad_shapes():
    # Large domains start their items from stored roots; small ones walk.
    assert hip_abi.dcf_expand_plan(1, 24, 0, 256)["top_G"] >= 0
    assert hip_abi.dcf_expand_plan(1, 12, 0, 256)["top_G"] == -1
    assert hip_abi.dcf_expand_plan(1, 20, 0, 256)["G"] > 0
    for args in ((0, 8, 0, 256), (1, 0, 0, 256), (1, 8, 8, 256), (1, 8, -1, 256), (1, 8, 0, 0),
                 (1, 64, 0, 256), (1 << 40, 30, 0, 256)):
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.dcf_expand_plan(*args)
        assert e.value.code == INVALID_ARGUMENT


# ---- the host API: every check before the device is touched, in order ---------
TYPE_MSG = "Value type T doesn't match parameters at `hierarchy_level`"
SHARD_MSG = "num_shards must be a power of two and 0 <= shard < num_shards"
MORE_SHARDS_MSG = "more shards than subtrees at this level"
WORDS_MSG = "`record_words` must be in [1, 1024]"
DB_MSG = "database buffer too small"
OUT_MSG = "device output buffer too small"
NULL_MSG = "`device_db` and `device_out` must not be null"
BATCH_MSG = "key batch does not match this DistributedComparisonFunction"


def _raised(call):
    with pytest.raises(D.DpfStatusError) as e:
        call()
    return e.value.code, e.value.message


def _bad_key(key):
    bad = type(key)()
    bad.CopyFrom(key)
    del bad.key.correction_words[-1]
    return bad


def _full(dcf, key, out, shard=0, num_shards=1):
    return dcf.evaluate_full_domain_to_device(key, out, shard=shard, num_shards=num_shards,
                                              stream=_NullStream())


def _dot(dcf, key, db, w, out, shard=0, num_shards=1):
    return dcf.evaluate_range_dot_to_device(key, db, w, out, shard=shard, num_shards=num_shards,
                                            stream=_NullStream())


def test_evaluates_full_domain_on_device_by_type():
    for vt, want in ((("int", 8), True), (("int", 64), True), (("xor", 128), True),
                     (("intmodn", 64, 18446744073709551557), False),
                     (("tuple", [("int", 32), ("int", 32)]), False)):
        assert make(vt, 6).evaluates_full_domain_on_device() is want, vt


def test_full_domain_to_device_reports_the_first_failing_check():
    """Two faults at once: key, shard arguments, buffer, value type."""
    dcf = make(("int", 64), 10)
    key = dcf.generate_keys(3, 1, seed_0=1, seed_1=2)[0]
    bad = _bad_key(key)
    key_msg = _raised(lambda: dcf.evaluate_packed(bad, [0]))[1]
    out = torch.zeros(8 << 10, dtype=torch.uint8)

    assert _raised(lambda: _full(dcf, bad, out, num_shards=3)) == (INVALID_ARGUMENT, key_msg)
    assert _raised(lambda: _full(dcf, key, out[:-1], num_shards=3)) == (INVALID_ARGUMENT, SHARD_MSG)
    for shard, num in ((2, 2), (-1, 2), (0, 0)):
        assert _raised(lambda: _full(dcf, key, out, shard, num)) == (INVALID_ARGUMENT, SHARD_MSG)
    assert _raised(lambda: _full(dcf, key, out[:-1], num_shards=1 << 10)) == \
        (INVALID_ARGUMENT, MORE_SHARDS_MSG)
    assert _raised(lambda: _full(dcf, key, out[:-1])) == (INVALID_ARGUMENT, OUT_MSG)
    assert _raised(lambda: _full(dcf, key, _Buffer(0, 8 << 10))) == (INVALID_ARGUMENT, OUT_MSG)
    # A shard's output is its share of the domain.
    assert _raised(lambda: _full(dcf, key, out[:(8 << 8) - 1], 1, 4)) == (INVALID_ARGUMENT, OUT_MSG)

    # An unsupported value type: after the buffer, and never a per-point answer.
    vt = ("intmodn", 64, 18446744073709551557)
    modn = make(vt, 6)
    mkey = modn.generate_keys(3, 1, seed_0=1, seed_1=2)[0]
    small = torch.zeros(8 << 6, dtype=torch.uint8)
    assert _raised(lambda: _full(modn, mkey, small[:-1])) == (INVALID_ARGUMENT, OUT_MSG)
    assert _raised(lambda: _full(modn, mkey, small, num_shards=3)) == (INVALID_ARGUMENT, SHARD_MSG)
    assert _raised(lambda: _full(modn, mkey, small))[0] == UNIMPLEMENTED
    assert _raised(lambda: modn.evaluate_full_domain_packed(mkey))[0] == UNIMPLEMENTED


def test_full_domain_packed_reports_the_first_failing_check():
    """Requested type, then key, then value type."""
    dcf = make(("int", 64), 10)
    key = dcf.generate_keys(3, 1, seed_0=1, seed_1=2)[0]
    bad = _bad_key(key)
    key_msg = _raised(lambda: dcf.evaluate_packed(bad, [0]))[1]
    assert _raised(lambda: dcf.evaluate_full_domain_packed(bad, D.integer_type(32))) == \
        (INVALID_ARGUMENT, TYPE_MSG)
    assert _raised(lambda: dcf.evaluate_full_domain_packed(bad)) == (INVALID_ARGUMENT, key_msg)
    modn = make(("intmodn", 64, 18446744073709551557), 6)
    mkey = modn.generate_keys(3, 1, seed_0=1, seed_1=2)[0]
    assert _raised(lambda: modn.evaluate_full_domain_packed(mkey, D.integer_type(64))) == \
        (INVALID_ARGUMENT, TYPE_MSG)
    assert _raised(lambda: modn.evaluate_full_domain_packed(_bad_key(mkey)))[0] == INVALID_ARGUMENT


def test_key_of_another_dcf_is_reported_before_the_shard_split():
    """The key check comes first for a key that is valid elsewhere, too (the
    batch call's counterpart needs a device batch: test_dcf_expand_gpu.py)."""
    dcf10, dcf6 = make(("int", 64), 10), make(("int", 64), 6)
    key6 = dcf6.generate_keys(3, 1, seed_0=1, seed_1=2)[0]
    out = torch.zeros(8 << 10, dtype=torch.uint8)
    # A key of another domain with a bad shard split: the key's error.
    code, msg = _raised(lambda: _full(dcf10, key6, out, num_shards=3))
    assert code == INVALID_ARGUMENT and msg != SHARD_MSG


def test_range_dot_to_device_reports_the_first_failing_check():
    """Two faults at once: key, shard split, record_words, database size,
    output size, null pointers, value type."""
    dcf = make(("int", 64), 10)
    key = dcf.generate_keys(3, 1, seed_0=1, seed_1=2)[0]
    bad = _bad_key(key)
    key_msg = _raised(lambda: dcf.evaluate_packed(bad, [0]))[1]
    db = torch.zeros(1 << 13, dtype=torch.uint8)        # 2^10 records of one uint64
    out = torch.zeros(8, dtype=torch.uint8)
    null_db = _Buffer(0, 1 << 13)

    assert _raised(lambda: _dot(dcf, bad, db, 0, out, num_shards=3)) == (INVALID_ARGUMENT, key_msg)
    assert _raised(lambda: _dot(dcf, key, db, 0, out, num_shards=3)) == (INVALID_ARGUMENT, SHARD_MSG)
    assert _raised(lambda: _dot(dcf, key, db, 0, out, num_shards=1 << 10)) == \
        (INVALID_ARGUMENT, MORE_SHARDS_MSG)
    for w in (0, -3, 1025):
        assert _raised(lambda: _dot(dcf, key, db[:-1], w, out)) == (INVALID_ARGUMENT, WORDS_MSG)
    assert _raised(lambda: _dot(dcf, key, db[:-1], 1, out[:7])) == (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _dot(dcf, key, db, 2, torch.zeros(16, dtype=torch.uint8))) == \
        (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _dot(dcf, key, db[:(1 << 11) - 1], 1, out, 1, 4)) == \
        (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _dot(dcf, key, null_db, 1, out[:7])) == (INVALID_ARGUMENT, OUT_MSG)
    assert _raised(lambda: _dot(dcf, key, null_db, 1, out)) == (INVALID_ARGUMENT, NULL_MSG)
    assert _raised(lambda: _dot(dcf, key, db, 1, _Buffer(0, 8))) == (INVALID_ARGUMENT, NULL_MSG)

    # Value types the fold is not defined for: after every buffer check.
    for vt in (("int", 32), ("xor", 64), ("intmodn", 64, 18446744073709551557)):
        other = make(vt, 10)
        okey = other.generate_keys(3, 1, seed_0=1, seed_1=2)[0]
        assert _raised(lambda: _dot(other, okey, null_db, 1, out)) == (INVALID_ARGUMENT, NULL_MSG)
        assert _raised(lambda: _dot(other, okey, db, 1, out))[0] == UNIMPLEMENTED
        assert _raised(lambda: other.evaluate_range_dot(okey, db, 1))[0] == UNIMPLEMENTED


def test_range_dot_reports_the_first_failing_check():
    """The host-returning call: key, record_words, database, value type."""
    dcf = make(("int", 64), 10)
    key = dcf.generate_keys(3, 1, seed_0=1, seed_1=2)[0]
    bad = _bad_key(key)
    key_msg = _raised(lambda: dcf.evaluate_packed(bad, [0]))[1]
    db = torch.zeros(1 << 13, dtype=torch.uint8)
    assert _raised(lambda: dcf.evaluate_range_dot(bad, db, 0)) == (INVALID_ARGUMENT, key_msg)
    assert _raised(lambda: dcf.evaluate_range_dot(key, db[:-1], 1025)) == \
        (INVALID_ARGUMENT, WORDS_MSG)
    assert _raised(lambda: dcf.evaluate_range_dot(key, db[:-1], 1)) == (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: dcf.evaluate_range_dot(key, _Buffer(0, 1 << 13), 1)) == \
        (INVALID_ARGUMENT, NULL_MSG)
