"""The batched database fold (EvaluateDotBatchToDevice / EvaluateDotBatch,
dpf_hip_dot_rows_batch) as far as it can be checked without a GPU: the C ABI's
symbols and signatures, the workspace size, every error the C ABI and the host
API detect before any device work, in their documented order (the database
and the output are fake non-null addresses), and the NumPy model the GPU tests
compare against."""
import ctypes
import inspect

import numpy as np
import pytest

import dot_batch_model as M
import oracle as O
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import pir
from distributed_point_functions_amd import proto as pb

INVALID_ARGUMENT, RESOURCE_EXHAUSTED, UNIMPLEMENTED = 3, 8, 12
U64, X64 = D.integer_type(64), D.xor_wrapper_type(64)
LOG_DOMAIN = 7
RECORDS = 1 << LOG_DOMAIN


def _desc(vt):
    return hip_abi.value_desc(O.leaves(vt), True, O.elements_per_block(vt), 1)


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


def _batch(dpf, keys, db, w, out, level=0, shard=0, num_shards=1):
    return dpf.evaluate_dot_batch_to_device(keys, level, db, w, out, shard=shard,
                                            num_shards=num_shards, stream=_NullStream())


def _raised(call):
    with pytest.raises(D.DpfStatusError) as e:
        call()
    return e.value.code, e.value.message


# ------------------------------------------------------------------- C ABI
def test_symbols_are_exported_and_declared():
    names = hip_abi.header_functions()
    lib = hip_abi.load()
    for f in ("dpf_hip_dot_rows_batch", "dpf_hip_dot_rows_batch_workspace_bytes",
              "dpf_hip_last_dot_batch_shape"):
        assert f in names
        assert hasattr(lib, f), f
    assert len(lib.dpf_hip_dot_rows_batch.argtypes) == 11
    assert len(lib.dpf_hip_dot_rows_batch_workspace_bytes.argtypes) == 3
    assert len(lib.dpf_hip_last_dot_batch_shape.argtypes) == 1
    assert len(hip_abi.last_dot_batch_shape()) == 3
    assert "#define DPF_HIP_DOT_BATCH_MAX_QUERIES 64" in open(hip_abi.HEADER).read()
    # The Python layers: the two methods, and the module's three functions.
    sig = inspect.signature(D.DistributedPointFunction.evaluate_dot_batch_to_device)
    assert list(sig.parameters) == ["self", "keys", "hierarchy_level", "db", "record_words", "out",
                                    "shard", "num_shards", "stream"]
    assert hasattr(D.DistributedPointFunction, "evaluate_dot_batch")
    assert list(inspect.signature(pir.query).parameters) == ["dpf", "rows", "beta", "root_seeds"]
    assert list(inspect.signature(pir.answer).parameters) == ["dpf", "keys", "db", "record_words",
                                                              "out", "stream"]
    assert list(inspect.signature(pir.reconstruct).parameters) == ["a0", "a1", "xor"]


@pytest.mark.parametrize("vt", [("int", 64), ("xor", 64)], ids=str)
def test_workspace_bytes_is_monotone(vt):
    desc = _desc(vt)
    size = lambda w, q: hip_abi.dot_batch_workspace_bytes(desc, w, q)   # noqa: E731
    assert size(1, 1) >= 8 and size(3, 17) >= 3 * 8 and size(1024, 64) >= 1024 * 8
    widths = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 1023, 1024)
    for q in (1, 2, 3, 4, 5, 8, 9, 16, 17, 63, 64):
        sizes = [size(w, q) for w in widths]
        assert sizes == sorted(sizes), (q, sizes)
    for w in widths:
        sizes = [size(w, q) for q in range(1, 65)]
        assert sizes == sorted(sizes), (w, sizes)


def test_workspace_bytes_rejects():
    lib = hip_abi.load()
    ok = _desc(("int", 64))
    for w, q in ((0, 1), (1025, 1), (1, 0), (1, 65), (-1, 1), (1, -1)):
        assert lib.dpf_hip_dot_rows_batch_workspace_bytes(ctypes.byref(ok), w, q) == -1
        msg = lib.dpf_hip_last_error().decode()
        assert ("record_words" if not 1 <= w <= 1024 else "num_queries") in msg
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.dot_batch_workspace_bytes(ok, w, q)
        assert e.value.code == INVALID_ARGUMENT
    for vt in (("xor", 128), ("int", 32), ("int", 128), ("xor", 32)):
        bad = _desc(vt)
        assert lib.dpf_hip_dot_rows_batch_workspace_bytes(ctypes.byref(bad), 1, 1) == -1
        msg = lib.dpf_hip_last_error().decode()
        assert "uint64_t and XorWrapper<uint64_t>" in msg
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.dot_batch_workspace_bytes(bad, 1, 1)
        assert e.value.code == UNIMPLEMENTED
    assert lib.dpf_hip_last_dot_batch_shape(None) == INVALID_ARGUMENT


def test_dot_rows_batch_rejects_arguments_before_any_device_work():
    """Counts, NULL pointers and the stride (3), then the type (12), then the
    workspace (8): the first failing check is the one reported."""
    lib = hip_abi.load()
    P = ctypes.c_void_p
    ok, bad = _desc(("int", 64)), _desc(("xor", 128))

    def call(rows=64, w=1, q=1, desc=ok, y=16, stride=512, db=16, ws=16, out=16):
        d = ctypes.byref(desc) if desc is not None else None
        st = lib.dpf_hip_dot_rows_batch(rows, w, q, d, P(y), stride, P(db), 0, P(ws), P(out), P(0))
        return st, lib.dpf_hip_last_error().decode()

    for w, q in ((0, 1), (1025, 1), (1, 0), (1, 65)):
        st, msg = call(w=w, q=q)
        assert st == INVALID_ARGUMENT
        assert ("record_words" if w != 1 else "num_queries") in msg
    assert call(rows=-1)[0] == INVALID_ARGUMENT
    for kw in ({"y": 0}, {"db": 0}, {"out": 0}, {"desc": None}):
        st, msg = call(**kw)
        assert (st, msg) == (INVALID_ARGUMENT, "NULL pointer"), kw
    # The stride: a multiple of 16, at least 8 * num_rows.
    for rows, stride in ((65, 512), (64, 520), (64, 504), (64, -512), (1, 8)):
        st, msg = call(rows=rows, stride=stride)
        assert st == INVALID_ARGUMENT and "y_stride_bytes" in msg, (rows, stride)
    st, msg = call(desc=bad)
    assert st == UNIMPLEMENTED and "uint64_t and XorWrapper<uint64_t>" in msg
    st, msg = call(ws=0)
    assert st == RESOURCE_EXHAUSTED
    assert str(hip_abi.dot_batch_workspace_bytes(ok, 1, 1)) in msg
    st, msg = call(w=33, q=17, ws=0, stride=512)
    assert st == RESOURCE_EXHAUSTED
    assert str(hip_abi.dot_batch_workspace_bytes(ok, 33, 17)) in msg
    # Two faults at once, in the documented order.
    assert call(w=0, desc=bad, ws=0)[0] == INVALID_ARGUMENT         # counts before the type
    assert call(out=0, desc=bad)[0] == INVALID_ARGUMENT             # pointers before the type
    assert call(stride=8, desc=bad, ws=0)[0] == INVALID_ARGUMENT    # stride before the type
    assert call(w=0, out=0)[1] == "record_words must be in [1, 1024]"
    assert call(out=0, stride=8)[1] == "NULL pointer"               # pointers before the stride
    assert call(desc=bad, ws=0)[0] == UNIMPLEMENTED                 # type before the workspace


# ---------------------------------------------------------------- host API
LEVEL_MSG = "`hierarchy_level` must be non-negative and less than parameters_.size()"
SHARD_MSG = "num_shards must be a power of two and 0 <= shard < num_shards"
MORE_SHARDS_MSG = "more shards than subtrees at this level"
WORDS_MSG = "`record_words` must be in [1, 1024]"
KEYS_MSG = "`keys` must hold between 1 and 64 keys"
DB_MSG = "database buffer too small"
OUT_MSG = "device output buffer too small"
NULL_MSG = "`device_db` and `device_out` must not be null"
TYPE_MSG = "the batched database fold is implemented for uint64_t and XorWrapper<uint64_t> only"


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
def test_host_errors_before_any_device_work(vt):
    dpf = _dpf(LOG_DOMAIN, vt)
    key = _key(dpf, vt)
    db, out = _db(), _out()
    # Where the condition is CheckSelectArgs', so is the message.
    sel = _dpf(LOG_DOMAIN, D.xor_wrapper_type(128))
    sel_key = _key(sel, D.xor_wrapper_type(128))

    def select_says(**kw):
        args = dict(keys=[sel_key], db=_Buffer(0x1000, RECORDS * 128 * 8), w=1, out=_out())
        args.update(kw)
        return _raised(lambda: sel.evaluate_select_to_device(
            args["keys"], args.get("level", 0), args["db"], args["w"], args["out"],
            shard=args.get("shard", 0), num_shards=args.get("num_shards", 1),
            stream=_NullStream()))

    for level in (1, -1):
        assert _raised(lambda: _batch(dpf, [key], db, 1, out, level=level)) == \
            select_says(level=level) == (INVALID_ARGUMENT, LEVEL_MSG)
    for shard, num in [(0, 3), (4, 4), (-1, 2), (0, 0)]:
        assert _raised(lambda: _batch(dpf, [key], db, 1, out, shard=shard, num_shards=num)) == \
            select_says(shard=shard, num_shards=num) == (INVALID_ARGUMENT, SHARD_MSG)
    assert _raised(lambda: _batch(dpf, [key], db, 1, out, num_shards=1 << LOG_DOMAIN)) == \
        (INVALID_ARGUMENT, MORE_SHARDS_MSG)
    for w in (0, -3, 1025):
        assert _raised(lambda: _batch(dpf, [key], db, w, out)) == select_says(w=w) == \
            (INVALID_ARGUMENT, WORDS_MSG)
    for keys in ([], [key] * 65):
        assert _raised(lambda: _batch(dpf, keys, db, 1, _out(65))) == (INVALID_ARGUMENT, KEYS_MSG)
        assert _raised(lambda: dpf.evaluate_dot_batch(keys, 0, db, 1)) == \
            (INVALID_ARGUMENT, KEYS_MSG)
    assert select_says(keys=[]) == (INVALID_ARGUMENT, KEYS_MSG)
    # The database: one record of W words per element of the shard.
    assert _raised(lambda: _batch(dpf, [key], _Buffer(0x1000, RECORDS * 8 - 1), 1, out)) == \
        (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _batch(dpf, [key], db, 2, _out(1, 2))) == (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _batch(dpf, [key], _Buffer(0x1000, RECORDS * 8 // 4 - 1), 1, out,
                                  shard=1, num_shards=4)) == (INVALID_ARGUMENT, DB_MSG)
    # The output: Q * W words.
    assert _raised(lambda: _batch(dpf, [key, key], db, 1, _Buffer(0x2000, 15))) == \
        (INVALID_ARGUMENT, OUT_MSG)
    for bad_db, bad_out in ((_Buffer(0, RECORDS * 8), out), (db, _Buffer(0, 8))):
        assert _raised(lambda: _batch(dpf, [key], bad_db, 1, bad_out)) == \
            (INVALID_ARGUMENT, NULL_MSG)
    # An invalid key: ValidateDpfKey's error, prefixed with the first failing index.
    bad = pb.DpfKey()
    bad.CopyFrom(key)
    del bad.correction_words[-1]
    key_msg = _raised(lambda: dpf.evaluate_at(bad, 0, [0]))[1]
    for call in (lambda: _batch(dpf, [key, key, bad, bad], db, 1, _out(4)),
                 lambda: dpf.evaluate_dot_batch([key, key, bad, bad], 0, db, 1)):
        assert _raised(call) == (INVALID_ARGUMENT, "DpfKey 2: " + key_msg)


def test_two_to_the_62_cap():
    big = _dpf(63, U64)
    key = _key(big, U64)
    want = _raised(lambda: big.evaluate_dot_to_device(key, 0, _db(), 1, _out(),
                                                      stream=_NullStream()))
    got = _raised(lambda: _batch(big, [key], _db(), 1, _out()))
    assert got == want and got[0] == INVALID_ARGUMENT and "2**62" in got[1]


@pytest.mark.parametrize("vt", [D.integer_type(32), D.integer_type(128), D.xor_wrapper_type(32),
                                D.xor_wrapper_type(128),
                                D.tuple_type(D.integer_type(64), D.integer_type(64))], ids=str)
def test_other_value_types_are_unimplemented(vt):
    dpf = _dpf(LOG_DOMAIN, vt)
    key = dpf.generate_keys_incremental(
        3, [D.to_value(vt, (1, 2) if vt.WhichOneof("type") == "tuple" else 1)], seeds=(1, 2))[0]
    for call in (lambda: _batch(dpf, [key], _db(4), 1, _out()),
                 lambda: dpf.evaluate_dot_batch([key], 0, _db(4), 1)):
        assert _raised(call) == (UNIMPLEMENTED, TYPE_MSG)


def test_reports_the_first_failing_check():
    """Two faults at once: the check that comes first in CheckDotBatchArgs is
    the one reported (level, unsupported type, shard split, record_words, key
    count, database size, output size, null pointers, key validation)."""
    dpf = _dpf(LOG_DOMAIN, U64)
    key = _key(dpf, U64)
    bad = pb.DpfKey()
    bad.CopyFrom(key)
    del bad.correction_words[-1]
    key_msg = _raised(lambda: dpf.evaluate_at(bad, 0, [0]))[1]
    db, out = _db(), _out()
    short_db = _Buffer(0x1000, RECORDS * 8 - 1)
    x128 = D.xor_wrapper_type(128)
    other = _dpf(LOG_DOMAIN, x128)
    other_key = _key(other, x128)

    assert _raised(lambda: _batch(other, [other_key], db, 1, out, level=1)) == \
        (INVALID_ARGUMENT, LEVEL_MSG)
    assert _raised(lambda: _batch(other, [other_key], db, 1, out, shard=0, num_shards=3)) == \
        (UNIMPLEMENTED, TYPE_MSG)
    assert _raised(lambda: _batch(dpf, [key], db, 0, out, shard=4, num_shards=4)) == \
        (INVALID_ARGUMENT, SHARD_MSG)
    assert _raised(lambda: _batch(dpf, [key], db, 0, out, num_shards=1 << LOG_DOMAIN)) == \
        (INVALID_ARGUMENT, MORE_SHARDS_MSG)
    assert _raised(lambda: _batch(dpf, [], db, 1025, out)) == (INVALID_ARGUMENT, WORDS_MSG)
    assert _raised(lambda: _batch(dpf, [key] * 65, short_db, 1, _out(65))) == \
        (INVALID_ARGUMENT, KEYS_MSG)
    assert _raised(lambda: _batch(dpf, [key, key], short_db, 1, _Buffer(0x2000, 15))) == \
        (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _batch(dpf, [key, key], _Buffer(0, RECORDS * 8), 1,
                                  _Buffer(0x2000, 15))) == (INVALID_ARGUMENT, OUT_MSG)
    assert _raised(lambda: _batch(dpf, [bad], _Buffer(0, RECORDS * 8), 1, out)) == \
        (INVALID_ARGUMENT, NULL_MSG)
    assert _raised(lambda: _batch(dpf, [key, bad], short_db, 1, _out(2))) == \
        (INVALID_ARGUMENT, DB_MSG)
    assert _raised(lambda: _batch(dpf, [key, bad], db, 1, _out(2))) == \
        (INVALID_ARGUMENT, "DpfKey 1: " + key_msg)
    # evaluate_dot_batch: the same checks on the whole domain.
    assert _raised(lambda: other.evaluate_dot_batch([other_key], 0, short_db, 0)) == \
        (UNIMPLEMENTED, TYPE_MSG)
    assert _raised(lambda: dpf.evaluate_dot_batch([key] * 65, 0, short_db, 1)) == \
        (INVALID_ARGUMENT, KEYS_MSG)
    assert _raised(lambda: dpf.evaluate_dot_batch([bad], 0, short_db, 1)) == \
        (INVALID_ARGUMENT, DB_MSG)


# ------------------------------------------------------------------- model
def test_model_hand_worked_case():
    """3 rows, 2 words, 2 queries, worked by hand with M = 2^64.
    uint64_t:
      q0: y = (1, 2, M-1) i.e. (1, 2, -1);  q1: y = (2^32, 0, 2^63)
      db = [[5, M-1], [2^63, 3], [7, 2^32 + 1]]
      out[0][0] = 5 + 2 * 2^63 - 7            = -2             (2^64 wraps to 0)
      out[0][1] = -1 + 6 - (2^32 + 1)         = 4 - 2^32
      out[1][0] = 5 * 2^32 + 7 * 2^63         = 5 * 2^32 + 2^63   (7 odd: one 2^63 stays)
      out[1][1] = -2^32 + 2^63 * (2^32 + 1)   = 2^63 - 2^32    (2^95 wraps to 0)
    XorWrapper<uint64_t>, the same numbers:
      out[0][0] = (1 & 5) ^ (2 & 2^63) ^ 7            = 1 ^ 0 ^ 7 = 6
      out[0][1] = 1 ^ (2 & 3) ^ (2^32 + 1)            = 1 ^ 2 ^ (2^32 + 1) = 2^32 + 2
      out[1][0] = (2^32 & 5) ^ 0 ^ (2^63 & 7)         = 0
      out[1][1] = 2^32 ^ 0 ^ (2^63 & (2^32 + 1))      = 2^32
    """
    Mod = 1 << 64
    y = np.array([[1, 2, Mod - 1], [1 << 32, 0, 1 << 63]], dtype=np.uint64)
    db = np.array([[5, Mod - 1], [1 << 63, 3], [7, (1 << 32) + 1]], dtype=np.uint64)
    want_add = np.array([[Mod - 2, Mod + 4 - (1 << 32)],
                         [5 * (1 << 32) + (1 << 63), (1 << 63) - (1 << 32)]], dtype=np.uint64)
    want_xor = np.array([[6, (1 << 32) + 2], [0, 1 << 32]], dtype=np.uint64)
    for f in (M.fold, M.fold_ints):
        assert np.array_equal(f(y, db, False), want_add), f.__name__
        assert np.array_equal(f(y, db, True), want_xor), f.__name__
    assert np.array_equal(M.combine(want_add, want_add, False),
                          np.array([[Mod - 4, Mod + 8 - (1 << 33)],
                                    [10 * (1 << 32), Mod - (1 << 33)]], dtype=np.uint64))
    assert not M.combine(want_xor, want_xor, True).any()


@pytest.mark.parametrize("xor", [False, True])
def test_model_wraparound_equals_python_ints(xor):
    rng = np.random.default_rng(7)
    y = rng.integers(0, 2**64, size=(3, 70), dtype=np.uint64)
    db = rng.integers(0, 2**64, size=(70, 5), dtype=np.uint64)
    assert np.array_equal(M.fold(y, db, xor), M.fold_ints(y, db, xor))
    # No rows: the empty sum.
    assert not M.fold(y[:, :0], db[:0], xor).any()
    # All-ones times all-ones rows: n * (2^64 - 1)^2 = n mod 2^64.
    ones = np.full((1, 1000), 2**64 - 1, dtype=np.uint64)
    if not xor:
        assert np.array_equal(M.fold(ones, ones.T.repeat(3, axis=1), False),
                              np.full((1, 3), 1000, dtype=np.uint64))


def test_pir_reconstruct():
    a = np.array([[2**64 - 1, 5]], dtype=np.uint64)
    b = np.array([[3, 2**63]], dtype=np.uint64)
    assert np.array_equal(pir.reconstruct(a, b, xor=False),
                          np.array([[2, 5 + 2**63]], dtype=np.uint64))
    assert np.array_equal(pir.reconstruct(a, b, xor=True), a ^ b)
    with pytest.raises(ValueError):
        pir.query(_dpf(LOG_DOMAIN, U64), [1, 2], beta=[1])
