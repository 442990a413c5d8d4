"""The database fold (EvaluateDotToDevice, dpf_hip_expand_dot / dpf_hip_dot_rows)
as far as it can be checked without a GPU: the C ABI's declarations, the
workspace size, and every error the host API detects before any device work."""
import os
import subprocess

import pytest
import torch

from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import proto as pb

INVALID_ARGUMENT, UNIMPLEMENTED = 3, 12


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
    return D.DistributedPointFunction.create(p)


def _key(dpf, vt, alpha=3, beta=1):
    return dpf.generate_keys_incremental(alpha, [D.to_value(vt, beta)], seeds=(1, 2))[0]


def _desc(kind, bits):
    return hip_abi.value_desc([(kind, bits, 0)], True, 128 // bits, 1)


def test_header_declares_the_dot_entry_points():
    names = hip_abi.header_functions()
    for f in ("dpf_hip_expand_dot", "dpf_hip_dot_rows", "dpf_hip_expand_dot_workspace_bytes",
              "dpf_hip_expand_dot_fused", "dpf_hip_last_dot_kernel"):
        assert f in names
    lib = hip_abi.load()
    for f in names:
        assert hasattr(lib, f), f
    assert hip_abi.last_dot_kernel() in ("", "small", "pair", "octet", "rows")


@pytest.mark.parametrize("kind,bits", [(hip_abi.LEAF_INT, 64), (hip_abi.LEAF_XOR, 64),
                                       (hip_abi.LEAF_XOR, 128)])
def test_workspace_bytes_positive_and_monotone(kind, bits):
    d = _desc(kind, bits)
    sizes = [hip_abi.dot_workspace_bytes(d, w) for w in (1, 2, 3, 4, 32, 33, 1023, 1024)]
    assert sizes[0] > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    # One partial row of W elements per workgroup must fit at least 256 times.
    assert sizes[-1] >= 256 * 1024 * bits // 8


def test_workspace_bytes_rejects_width_and_type():
    d = _desc(hip_abi.LEAF_INT, 64)
    for w in (0, -1, 1025):
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.dot_workspace_bytes(d, w)
        assert e.value.code == INVALID_ARGUMENT
    for kind, bits in ((hip_abi.LEAF_INT, 32), (hip_abi.LEAF_INT, 128), (hip_abi.LEAF_XOR, 32)):
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.dot_workspace_bytes(_desc(kind, bits), 1)
        assert e.value.code == UNIMPLEMENTED
        assert "uint64_t, XorWrapper<uint64_t> and XorWrapper<absl::uint128>" in str(e.value)
    assert hip_abi.load().dpf_hip_expand_dot_fused(None, 1) == 0


def _dot(dpf, key, db, w, out, level=0, shard=0, num_shards=1):
    return dpf.evaluate_dot_to_device(key, level, db, w, out, shard=shard, num_shards=num_shards,
                                      stream=_NullStream())


def test_host_errors_before_any_device_work():
    vt = D.integer_type(64)
    dpf = _dpf(10, vt)
    key = _key(dpf, vt)
    db = torch.zeros(1 << 13, dtype=torch.uint8)       # 2^10 records of one uint64
    out = torch.zeros(8, dtype=torch.uint8)

    # Shard arguments and hierarchy level: EvaluateShardToDevice's status and message.
    ctx_buf = torch.zeros(1 << 13, dtype=torch.uint8)
    for shard, num in [(0, 3), (4, 4), (-1, 2), (0, 0), (0, 1 << 10)]:
        with pytest.raises(D.DpfStatusError) as want:
            dpf.evaluate_shard_to_device(0, shard, num, dpf.create_evaluation_context(key),
                                         ctx_buf, stream=_NullStream())
        with pytest.raises(D.DpfStatusError) as e:
            _dot(dpf, key, db, 1, out, shard=shard, num_shards=num)
        assert (e.value.code, e.value.message) == (want.value.code, want.value.message)
        assert e.value.code == INVALID_ARGUMENT
    for level in (1, -1):
        with pytest.raises(D.DpfStatusError) as want:
            dpf.evaluate_shard_to_device(level, 0, 1, dpf.create_evaluation_context(key), ctx_buf,
                                         stream=_NullStream())
        with pytest.raises(D.DpfStatusError) as e:
            _dot(dpf, key, db, 1, out, level=level)
        assert (e.value.code, e.value.message) == (want.value.code, want.value.message)
        assert "hierarchy_level" in e.value.message

    for w in (0, -3, 1025):
        with pytest.raises(D.DpfStatusError) as e:
            _dot(dpf, key, db, w, out)
        assert e.value.code == INVALID_ARGUMENT and "record_words" in e.value.message

    with pytest.raises(D.DpfStatusError) as e:
        _dot(dpf, key, db[:-1], 1, out)
    assert (e.value.code, e.value.message) == (INVALID_ARGUMENT, "database buffer too small")
    with pytest.raises(D.DpfStatusError) as e:
        _dot(dpf, key, db, 2, torch.zeros(16, dtype=torch.uint8))
    assert e.value.message == "database buffer too small"
    # A shard's database is its share of the records.
    with pytest.raises(D.DpfStatusError) as e:
        _dot(dpf, key, db[:(1 << 11) - 1], 1, out, shard=1, num_shards=4)
    assert e.value.message == "database buffer too small"

    with pytest.raises(D.DpfStatusError) as e:
        _dot(dpf, key, db, 1, out[:7])
    assert (e.value.code, e.value.message) == (INVALID_ARGUMENT, "device output buffer too small")

    for bad_db, bad_out in ((_Buffer(0, 1 << 13), out), (db, _Buffer(0, 8))):
        with pytest.raises(D.DpfStatusError) as e:
            _dot(dpf, key, bad_db, 1, bad_out)
        assert e.value.code == INVALID_ARGUMENT and "null" in e.value.message

    # An invalid key: ValidateDpfKey's error, the one EvaluateAt reports.
    bad = pb.DpfKey()
    bad.CopyFrom(key)
    del bad.correction_words[-1]
    with pytest.raises(D.DpfStatusError) as want:
        dpf.evaluate_at(bad, 0, [0])
    with pytest.raises(D.DpfStatusError) as e:
        _dot(dpf, bad, db, 1, out)
    assert (e.value.code, e.value.message) == (want.value.code, want.value.message)
    assert e.value.code == INVALID_ARGUMENT


@pytest.mark.parametrize("vt", [D.integer_type(32), D.integer_type(128),
                                D.tuple_type(D.integer_type(64), D.integer_type(64)),
                                D.int_mod_n_type(64, 18446744073709551557)], ids=str)
def test_unsupported_value_types_are_unimplemented(vt):
    dpf = _dpf(6, vt)
    dpf.register_value_type(vt)
    key = dpf.generate_keys_incremental(
        3, [D.to_value(vt, (1, 2) if vt.WhichOneof("type") == "tuple" else 1)], seeds=(1, 2))[0]
    db = torch.zeros(1 << 12, dtype=torch.uint8)
    out = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(D.DpfStatusError) as e:
        _dot(dpf, key, db, 1, out)
    assert e.value.code == UNIMPLEMENTED
    assert "uint64_t, XorWrapper<uint64_t> and XorWrapper<absl::uint128>" in e.value.message
    with pytest.raises(D.DpfStatusError) as e:
        dpf.evaluate_dot(key, 0, db, 1)
    assert e.value.code == UNIMPLEMENTED


LEVEL_MSG = "`hierarchy_level` must be non-negative and less than parameters_.size()"
SHARD_MSG = "num_shards must be a power of two and 0 <= shard < num_shards"
MORE_SHARDS_MSG = "more shards than subtrees at this level"
WORDS_MSG = "`record_words` must be in [1, 1024]"
DB_MSG = "database buffer too small"
OUT_MSG = "device output buffer too small"
NULL_MSG = "`device_db` and `device_out` must not be null"


def _without_last_correction_word(key):
    bad = pb.DpfKey()
    bad.CopyFrom(key)
    del bad.correction_words[-1]
    return bad


def _raised(call):
    with pytest.raises(D.DpfStatusError) as e:
        call()
    return e.value.code, e.value.message


def test_evaluate_dot_to_device_reports_the_first_failing_check():
    """Two faults at once: the check that comes first in EvaluateDotToDevice is
    the one reported (level, shard split, record_words, database size, output
    size, null pointers, key validation, unsupported type)."""
    vt = D.integer_type(64)
    dpf = _dpf(10, vt)
    key = _key(dpf, vt)
    bad = _without_last_correction_word(key)
    key_msg = _raised(lambda: dpf.evaluate_at(bad, 0, [0]))[1]
    db = torch.zeros(1 << 13, dtype=torch.uint8)
    out = torch.zeros(8, dtype=torch.uint8)
    null_db = _Buffer(0, 1 << 13)

    assert _raised(lambda: _dot(dpf, key, db, 1, out, level=1, shard=0, num_shards=3)) == \
        (INVALID_ARGUMENT, LEVEL_MSG)
    assert _raised(lambda: _dot(dpf, key, db, 0, out, shard=0, num_shards=3)) == \
        (INVALID_ARGUMENT, SHARD_MSG)
    assert _raised(lambda: _dot(dpf, key, db, 0, out, num_shards=1 << 10)) == \
        (INVALID_ARGUMENT, MORE_SHARDS_MSG)
    assert _raised(lambda: _dot(dpf, key, db[:-1], 1025, out)) == (INVALID_ARGUMENT, WORDS_MSG)
    assert _raised(lambda: _dot(dpf, key, db[:-1], 1, out[:7])) == (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _dot(dpf, key, null_db, 1, out[:7])) == (INVALID_ARGUMENT, OUT_MSG)
    assert _raised(lambda: _dot(dpf, bad, null_db, 1, out)) == (INVALID_ARGUMENT, NULL_MSG)
    assert _raised(lambda: _dot(dpf, bad, db[:-1], 1, out)) == (INVALID_ARGUMENT, DB_MSG)

    # An invalid key of a value type the fold does not support: the key's error.
    v32 = D.integer_type(32)
    dpf32 = _dpf(6, v32)
    bad32 = _without_last_correction_word(_key(dpf32, v32))
    key32_msg = _raised(lambda: dpf32.evaluate_at(bad32, 0, [0]))[1]
    assert _raised(lambda: _dot(dpf32, bad32, db, 1, out)) == (INVALID_ARGUMENT, key32_msg)
    assert _raised(lambda: _dot(dpf, bad, db, 1, out)) == (INVALID_ARGUMENT, key_msg)
    # ... and a short database with it: the database's.
    assert _raised(lambda: _dot(dpf32, bad32, db[:255], 1, out)) == (INVALID_ARGUMENT, DB_MSG)


def test_evaluate_dot_reports_the_first_failing_check():
    """EvaluateDotPacked's order: level, record_words, null database,
    unsupported type, database size, key validation.  evaluate_dot passes no
    requested type; test_evaluate_dot_template_type_check_comes_second has
    that check, through the C++ template."""
    vt = D.integer_type(64)
    dpf = _dpf(10, vt)
    key = _key(dpf, vt)
    bad = _without_last_correction_word(key)
    key_msg = _raised(lambda: dpf.evaluate_at(bad, 0, [0]))[1]
    db = torch.zeros(1 << 13, dtype=torch.uint8)
    null_db = _Buffer(0, 1 << 13)
    v32 = D.integer_type(32)
    dpf32 = _dpf(6, v32)
    key32 = _key(dpf32, v32)

    assert _raised(lambda: dpf.evaluate_dot(key, 1, db, 0)) == (INVALID_ARGUMENT, LEVEL_MSG)
    assert _raised(lambda: dpf.evaluate_dot(key, 0, null_db, 1025)) == (INVALID_ARGUMENT, WORDS_MSG)
    assert _raised(lambda: dpf32.evaluate_dot(key32, 0, null_db, 1)) == (INVALID_ARGUMENT, NULL_MSG)
    code, msg = _raised(lambda: dpf32.evaluate_dot(key32, 0, db[:255], 1))
    assert code == UNIMPLEMENTED
    assert "uint64_t, XorWrapper<uint64_t> and XorWrapper<absl::uint128>" in msg
    assert _raised(lambda: dpf.evaluate_dot(bad, 0, db[:-1], 1)) == (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: dpf.evaluate_dot(bad, 0, db, 1)) == (INVALID_ARGUMENT, key_msg)


def test_evaluate_dot_template_type_check_comes_second(tmp_path):
    """EvaluateDot<T> with a T that is not the level's type: reported after a
    bad level and before bad record_words, a null or a short database
    (tests/cpp/dot_type_precedence_test.cc; host errors only, no GPU calls)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "distributed_point_functions_amd", "lib")
    exe = tmp_path / "dot_type_precedence_test"
    subprocess.run(["g++", "-O1", "-std=c++20", "-Wall", f"-I{os.path.join(root, 'include')}",
                    os.path.join(root, "tests", "cpp", "dot_type_precedence_test.cc"),
                    "-o", str(exe), f"-L{lib}", "-ldpf", "-ldpf_hip", f"-Wl,-rpath,{lib}"],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
