"""The bit-selected database fold (EvaluateSelectToDevice / EvaluateSelect,
dpf_hip_select_rows) as far as it can be checked without a GPU: the C ABI's
symbols, the workspace size, and every error the host API detects before any
device work (the database and the output are fake non-null addresses)."""
import ctypes

import pytest

from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import proto as pb

INVALID_ARGUMENT, UNIMPLEMENTED = 3, 12
X128 = D.xor_wrapper_type(128)
LOG_DOMAIN = 6                      # 2^6 blocks of 128 records
RECORDS = (1 << LOG_DOMAIN) * 128


class _NullStream:
    cuda_stream = 0


class _Buffer:
    """Stands in for a device tensor: an address and a size, never read."""

    def __init__(self, ptr, nbytes):
        self._ptr, self._n = ptr, nbytes

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n

    def element_size(self):
        return 1


def _dpf(log_domain, vt):
    p = pb.DpfParameters(log_domain_size=log_domain)
    p.value_type.CopyFrom(vt)
    dpf = D.DistributedPointFunction.create(p)
    dpf.register_value_type(vt)
    return dpf


def _key(dpf, vt, alpha=3, beta=1):
    return dpf.generate_keys_incremental(alpha, [D.to_value(vt, beta)], seeds=(1, 2))[0]


def _db(record_words=1, records=RECORDS):
    return _Buffer(0x1000, records * record_words * 8)


def _out(num_keys=1, record_words=1):
    return _Buffer(0x2000, num_keys * record_words * 8)


def _select(dpf, keys, db, w, out, level=0, shard=0, num_shards=1):
    return dpf.evaluate_select_to_device(keys, level, db, w, out, shard=shard,
                                         num_shards=num_shards, stream=_NullStream())


def test_symbols_are_exported_and_declared():
    names = hip_abi.header_functions()
    lib = hip_abi.load()
    for f in ("dpf_hip_select_rows", "dpf_hip_select_workspace_bytes",
              "dpf_hip_last_select_shape"):
        assert f in names
        assert hasattr(lib, f), f
    assert len(hip_abi.last_select_shape()) == 3


def test_workspace_bytes():
    sizes = {(w, q): hip_abi.select_workspace_bytes(w, q) for w, q in ((1, 1), (1024, 64), (3, 17))}
    assert all(n > 0 for n in sizes.values())
    # At least one partial [tile][W] of uint64 behind the header, tile >= 1.
    assert sizes[1, 1] >= 8 and sizes[1024, 64] >= 1024 * 8 and sizes[3, 17] >= 3 * 8
    lib = hip_abi.load()
    for w, q in ((0, 1), (1025, 1), (1, 0), (1, 65)):
        assert lib.dpf_hip_select_workspace_bytes(w, q) == -1
        msg = lib.dpf_hip_last_error().decode()
        assert ("record_words" if w in (0, 1025) else "num_queries") in msg
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.select_workspace_bytes(w, q)
        assert e.value.code == INVALID_ARGUMENT


def test_select_rows_rejects_arguments_before_any_device_work():
    lib = hip_abi.load()
    P = ctypes.c_void_p
    for w, q in ((0, 1), (1025, 1), (1, 0), (1, 65)):
        st = lib.dpf_hip_select_rows(64, w, q, P(16), 16, P(16), 0, P(16), P(16), P(0))
        assert st == INVALID_ARGUMENT
        assert lib.dpf_hip_last_error().decode()
    # The stride: a multiple of 16, at least ceil(num_rows / 8).
    for rows, stride in ((129, 16), (64, 8), (64, 24)):
        assert lib.dpf_hip_select_rows(rows, 1, 1, P(16), stride, P(16), 0, P(16), P(16),
                                       P(0)) == INVALID_ARGUMENT
        assert "sel_stride_bytes" in lib.dpf_hip_last_error().decode()
    assert lib.dpf_hip_select_rows(64, 1, 1, P(0), 16, P(16), 0, P(16), P(16),
                                   P(0)) == INVALID_ARGUMENT


def test_host_errors_before_any_device_work():
    dpf = _dpf(LOG_DOMAIN, X128)
    key = _key(dpf, X128)
    db, out = _db(), _out()

    # Level and shard arguments: EvaluateDotToDevice's status and message.
    for level in (1, -1):
        with pytest.raises(D.DpfStatusError) as want:
            dpf.evaluate_dot_to_device(key, level, db, 1, out, stream=_NullStream())
        with pytest.raises(D.DpfStatusError) as e:
            _select(dpf, [key], db, 1, out, level=level)
        assert (e.value.code, e.value.message) == (want.value.code, want.value.message)
        assert e.value.code == INVALID_ARGUMENT and "hierarchy_level" in e.value.message
    for shard, num in [(0, 3), (4, 4), (-1, 2), (0, 0), (0, 1 << 7)]:
        with pytest.raises(D.DpfStatusError) as want:
            dpf.evaluate_dot_to_device(key, 0, db, 1, out, shard=shard, num_shards=num,
                                       stream=_NullStream())
        with pytest.raises(D.DpfStatusError) as e:
            _select(dpf, [key], db, 1, out, shard=shard, num_shards=num)
        assert (e.value.code, e.value.message) == (want.value.code, want.value.message)
        assert e.value.code == INVALID_ARGUMENT
    # One shard per tree leaf is the most.
    with pytest.raises(D.DpfStatusError) as e:
        _select(dpf, [key], db, 1, out, num_shards=1 << (LOG_DOMAIN + 1))
    assert e.value.message == "more shards than subtrees at this level"

    for w in (0, -3, 1025):
        with pytest.raises(D.DpfStatusError) as e:
            _select(dpf, [key], db, w, out)
        assert (e.value.code, e.value.message) == (INVALID_ARGUMENT,
                                                   "`record_words` must be in [1, 1024]")

    # The database: one record per output bit, whatever the value type's width.
    with pytest.raises(D.DpfStatusError) as e:
        _select(dpf, [key], _Buffer(0x1000, RECORDS * 8 - 1), 1, out)
    assert (e.value.code, e.value.message) == (INVALID_ARGUMENT, "database buffer too small")
    with pytest.raises(D.DpfStatusError) as e:
        _select(dpf, [key], db, 2, _out(1, 2))
    assert e.value.message == "database buffer too small"
    with pytest.raises(D.DpfStatusError) as e:     # a shard's database is its share
        _select(dpf, [key], _Buffer(0x1000, RECORDS * 8 // 4 - 1), 1, out, shard=1, num_shards=4)
    assert e.value.message == "database buffer too small"

    # The output: Q * W words.
    with pytest.raises(D.DpfStatusError) as e:
        _select(dpf, [key, key], db, 1, _Buffer(0x2000, 15))
    assert (e.value.code, e.value.message) == (INVALID_ARGUMENT, "device output buffer too small")

    for bad_db, bad_out in ((_Buffer(0, RECORDS * 8), out), (db, _Buffer(0, 8))):
        with pytest.raises(D.DpfStatusError) as e:
            _select(dpf, [key], bad_db, 1, bad_out)
        assert e.value.code == INVALID_ARGUMENT and "null" in e.value.message

    # The keys: 1 to 64 of them.
    for keys in ([], [key] * 65):
        with pytest.raises(D.DpfStatusError) as e:
            _select(dpf, keys, db, 1, _out(65))
        assert e.value.code == INVALID_ARGUMENT and "keys" in e.value.message
        with pytest.raises(D.DpfStatusError) as e:
            dpf.evaluate_select(keys, 0, db, 1)
        assert e.value.code == INVALID_ARGUMENT and "keys" in e.value.message

    # An invalid key: ValidateDpfKey's error, prefixed with the first failing index.
    bad = pb.DpfKey()
    bad.CopyFrom(key)
    del bad.correction_words[-1]
    with pytest.raises(D.DpfStatusError) as want:
        dpf.evaluate_at(bad, 0, [0])
    for call in (lambda: _select(dpf, [key, key, bad, bad], db, 1, _out(4)),
                 lambda: dpf.evaluate_select([key, key, bad, bad], 0, db, 1)):
        with pytest.raises(D.DpfStatusError) as e:
            call()
        assert e.value.code == want.value.code == INVALID_ARGUMENT
        assert e.value.message == "DpfKey 2: " + want.value.message


def test_evaluate_select_host_errors():
    dpf = _dpf(LOG_DOMAIN, X128)
    key = _key(dpf, X128)
    for level in (1, -1):
        with pytest.raises(D.DpfStatusError) as e:
            dpf.evaluate_select([key], level, _db(), 1)
        assert e.value.code == INVALID_ARGUMENT and "hierarchy_level" in e.value.message
    for w in (0, 1025):
        with pytest.raises(D.DpfStatusError) as e:
            dpf.evaluate_select([key], 0, _db(), w)
        assert e.value.message == "`record_words` must be in [1, 1024]"
    with pytest.raises(D.DpfStatusError) as e:
        dpf.evaluate_select([key], 0, _Buffer(0x1000, RECORDS * 8 - 1), 1)
    assert e.value.message == "database buffer too small"
    with pytest.raises(D.DpfStatusError) as e:
        dpf.evaluate_select([key], 0, _Buffer(0, RECORDS * 8), 1)
    assert e.value.code == INVALID_ARGUMENT and "null" in e.value.message


def test_two_to_the_62_cap_counts_records():
    # 2^56 blocks of 128 records: the share vector (2^56 elements) is under
    # the cap, the records (2^63) are not.
    dpf = _dpf(56, X128)
    key = _key(dpf, X128)
    big = _dpf(63, X128)
    with pytest.raises(D.DpfStatusError) as want:     # EvaluateDotToDevice's message
        big.evaluate_dot_to_device(_key(big, X128), 0, _db(), 1, _out(), stream=_NullStream())
    with pytest.raises(D.DpfStatusError) as e:
        _select(dpf, [key], _db(), 1, _out())
    assert e.value.code == INVALID_ARGUMENT
    assert e.value.message == want.value.message and "2**62" in e.value.message


@pytest.mark.parametrize("vt", [D.integer_type(64), D.integer_type(32), D.integer_type(128),
                                D.xor_wrapper_type(32),
                                D.tuple_type(D.integer_type(64), D.integer_type(64))], ids=str)
def test_other_value_types_are_unimplemented(vt):
    dpf = _dpf(LOG_DOMAIN, vt)
    key = dpf.generate_keys_incremental(
        3, [D.to_value(vt, (1, 2) if vt.WhichOneof("type") == "tuple" else 1)], seeds=(1, 2))[0]
    for call in (lambda: _select(dpf, [key], _db(), 1, _out()),
                 lambda: dpf.evaluate_select([key], 0, _db(), 1)):
        with pytest.raises(D.DpfStatusError) as e:
            call()
        assert e.value.code == UNIMPLEMENTED
        assert "XorWrapper<uint64_t> and XorWrapper<absl::uint128>" in e.value.message


LEVEL_MSG = "`hierarchy_level` must be non-negative and less than parameters_.size()"
SHARD_MSG = "num_shards must be a power of two and 0 <= shard < num_shards"
MORE_SHARDS_MSG = "more shards than subtrees at this level"
WORDS_MSG = "`record_words` must be in [1, 1024]"
KEYS_MSG = "`keys` must hold between 1 and 64 keys"
DB_MSG = "database buffer too small"
OUT_MSG = "device output buffer too small"
NULL_MSG = "`device_db` and `device_out` must not be null"
TYPE_MSG = ("the bit-selected database fold is implemented for XorWrapper<uint64_t> and "
            "XorWrapper<absl::uint128> only")


def _raised(call):
    with pytest.raises(D.DpfStatusError) as e:
        call()
    return e.value.code, e.value.message


def test_select_reports_the_first_failing_check():
    """Two faults at once: the check that comes first in CheckSelectArgs is the
    one reported (level, unsupported type, shard split, record_words, key
    count, database size, output size, null pointers, key validation)."""
    dpf = _dpf(LOG_DOMAIN, X128)
    key = _key(dpf, X128)
    bad = pb.DpfKey()
    bad.CopyFrom(key)
    del bad.correction_words[-1]
    key_msg = _raised(lambda: dpf.evaluate_at(bad, 0, [0]))[1]
    db, out = _db(), _out()
    short_db = _Buffer(0x1000, RECORDS * 8 - 1)
    u64 = D.integer_type(64)
    other = _dpf(LOG_DOMAIN, u64)
    other_key = _key(other, u64)

    assert _raised(lambda: _select(other, [other_key], db, 1, out, level=1)) == \
        (INVALID_ARGUMENT, LEVEL_MSG)
    assert _raised(lambda: _select(other, [other_key], db, 1, out, shard=0, num_shards=3)) == \
        (UNIMPLEMENTED, TYPE_MSG)
    assert _raised(lambda: _select(dpf, [key], db, 0, out, shard=4, num_shards=4)) == \
        (INVALID_ARGUMENT, SHARD_MSG)
    assert _raised(lambda: _select(dpf, [key], db, 0, out, num_shards=1 << (LOG_DOMAIN + 1))) == \
        (INVALID_ARGUMENT, MORE_SHARDS_MSG)
    assert _raised(lambda: _select(dpf, [], db, 1025, out)) == (INVALID_ARGUMENT, WORDS_MSG)
    assert _raised(lambda: _select(dpf, [key] * 65, short_db, 1, _out(65))) == \
        (INVALID_ARGUMENT, KEYS_MSG)
    assert _raised(lambda: _select(dpf, [key, key], short_db, 1, _Buffer(0x2000, 15))) == \
        (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _select(dpf, [key, key], _Buffer(0, RECORDS * 8), 1,
                                   _Buffer(0x2000, 15))) == (INVALID_ARGUMENT, OUT_MSG)
    assert _raised(lambda: _select(dpf, [bad], _Buffer(0, RECORDS * 8), 1, out)) == \
        (INVALID_ARGUMENT, NULL_MSG)
    assert _raised(lambda: _select(dpf, [key, bad], short_db, 1, _out(2))) == \
        (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _select(dpf, [key, bad], db, 1, _out(2))) == \
        (INVALID_ARGUMENT, "DpfKey 1: " + key_msg)
    # evaluate_select: the same checks on the whole domain.
    assert _raised(lambda: other.evaluate_select([other_key], 0, short_db, 0)) == \
        (UNIMPLEMENTED, TYPE_MSG)
    assert _raised(lambda: dpf.evaluate_select([key] * 65, 0, short_db, 1)) == \
        (INVALID_ARGUMENT, KEYS_MSG)
    assert _raised(lambda: dpf.evaluate_select([bad], 0, short_db, 1)) == (INVALID_ARGUMENT, DB_MSG)
