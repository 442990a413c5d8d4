"""Multi-query PIR over a bucketed database (dpf_hip_expand_rows,
dpf_hip_dot_buckets, EvaluateDotBuckets[ToDevice]) as far as it can be checked
without a GPU: the C ABI's declarations, the supported types, the argument
checks of both entry points and their order, the expansion's launch plan, the
fold's workspace size and the order of the host API's checks."""
import ctypes
import re

import pytest
import torch

from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from test_key_batch_cpu import make

INVALID_ARGUMENT, RESOURCE_EXHAUSTED, UNIMPLEMENTED = 3, 8, 12
SYMBOLS = ("dpf_hip_expand_rows", "dpf_hip_expand_rows_supported", "dpf_hip_expand_rows_plan",
           "dpf_hip_dot_buckets", "dpf_hip_last_dot_buckets_shape")
ITEMS_PER_CU = 256
MODN = 18446744073709551557


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
    assert "dpf_hip_dot_buckets_workspace_bytes" in names
    assert lib.dpf_hip_dot_buckets_workspace_bytes.restype is ctypes.c_int64
    assert lib.dpf_hip_abi_version() == 2


def test_supported_types():
    for kind in (hip_abi.LEAF_INT, hip_abi.LEAF_XOR):
        assert hip_abi.expand_rows_supported(_desc(kind, 64))
        for bits in (8, 16, 32, 128):
            assert not hip_abi.expand_rows_supported(_desc(kind, bits)), (kind, bits)
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    for d in (modn, pair, None):
        assert not hip_abi.expand_rows_supported(d)


_RAW = (ctypes.c_uint64 * 66)()
_BASE = (ctypes.addressof(_RAW) + 15) & ~15     # a 16-byte aligned dummy, never read
_P = ctypes.c_void_p(_BASE)


def _ptr(obj):
    return ctypes.cast(ctypes.pointer(obj), ctypes.c_void_p)


# ---- dpf_hip_expand_rows ------------------------------------------------------------
def _stable_id(over):
    """str(over), with ctypes pointers and arrays named by what they hold, not
    by their address: the same test id in every process."""
    def show(v):
        if isinstance(v, ctypes.c_void_p):
            return f"base+{v.value - _BASE}"
        if isinstance(v, ctypes.Array):
            return f"begin{list(v)}"
        return repr(v)
    return "{" + ", ".join(f"{k!r}: {show(v)}" for k, v in over.items()) + "}"


def _rows(desc=None, null_desc=False, **over):
    """A call of dpf_hip_expand_rows whose pointers are non-null, 16-byte
    aligned dummies: it must be rejected before anything dereferences them."""
    lib = hip_abi.load()
    key = hip_abi.aes_key(0)
    d = desc if desc is not None else _desc(hip_abi.LEAF_INT, 64)
    a = dict(num_keys=2, num_levels=7, cw_stride=7, log_domain_size=8, key_seed=_P, party=_P,
             cw_seed=_P, cw_left=_P, cw_right=_P, kl=_ptr(key), kr=_ptr(key), kv=_ptr(key),
             desc=_ptr(d), vcw=_P, rows=_P, stride=8 << 8, stream=None)
    a.update(over)
    if null_desc:
        a["desc"] = None
    st = lib.dpf_hip_expand_rows(*a.values())
    return st, lib.dpf_hip_last_error().decode()


@pytest.mark.parametrize("over", [
    dict(num_keys=-1), dict(num_keys=1 << 31), dict(log_domain_size=0, num_levels=-1),
    dict(log_domain_size=25, num_levels=24, stride=8 << 25), dict(num_levels=8),
    dict(num_levels=6), dict(kl=None), dict(kr=None), dict(kv=None), dict(null_desc=True),
    dict(cw_stride=6), dict(stride=(8 << 8) - 16), dict(stride=(8 << 8) + 8), dict(stride=-16),
    dict(key_seed=None), dict(party=None), dict(cw_seed=None), dict(cw_left=None),
    dict(cw_right=None), dict(vcw=None), dict(rows=None),
    dict(rows=ctypes.c_void_p(_BASE + 8)),
], ids=_stable_id)
def test_expand_rows_argument_errors_are_invalid_argument(over):
    st, msg = _rows(**over)
    assert st == INVALID_ARGUMENT and msg


def test_expand_rows_unsupported_types_are_unimplemented():
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    for d in (modn, pair, _desc(hip_abi.LEAF_INT, 32), _desc(hip_abi.LEAF_XOR, 128)):
        assert _rows(desc=d)[0] == UNIMPLEMENTED


def test_expand_rows_two_faults_report_the_earlier_check():
    """Counts and domain, NULL descriptor or AES key, value type, cw_stride,
    the row stride, the empty batch, NULL arrays, alignment."""
    u32 = _desc(hip_abi.LEAF_INT, 32)
    # 1 before 2 and 3.
    assert "num_keys" in _rows(num_keys=-1, kl=None, desc=u32)[1]
    assert "log_domain_size" in _rows(log_domain_size=0, num_levels=-1, desc=u32)[1]
    # 2 before 3: a NULL AES key with an unsupported type.
    assert _rows(kl=None, desc=u32)[0] == INVALID_ARGUMENT
    # 3 before 4: an unsupported type with a short cw_stride.
    assert _rows(desc=u32, cw_stride=0)[0] == UNIMPLEMENTED
    # 4 before 5: a short cw_stride with a short row stride.
    assert "cw_stride" in _rows(cw_stride=0, stride=16)[1]
    # 5 before 6: a bad stride is an error even for an empty batch; so are 3 and 4.
    st, msg = _rows(num_keys=0, stride=16)
    assert st == INVALID_ARGUMENT and "row_stride_bytes" in msg
    assert _rows(num_keys=0, desc=u32)[0] == UNIMPLEMENTED
    assert _rows(num_keys=0, cw_stride=6)[0] == INVALID_ARGUMENT
    # 6 before 7: an empty batch returns OK whatever the arrays.
    assert _rows(num_keys=0, key_seed=None, party=None, rows=None)[0] == 0
    # 7 before 8: a NULL array with misaligned rows.
    st, msg = _rows(party=None, rows=ctypes.c_void_p(_BASE + 8))
    assert st == INVALID_ARGUMENT and "NULL" in msg
    st, msg = _rows(rows=ctypes.c_void_p(_BASE + 8))
    assert st == INVALID_ARGUMENT and "aligned" in msg


def test_expand_rows_no_tree_needs_no_correction_words():
    assert _rows(num_keys=0, log_domain_size=1, num_levels=0, cw_stride=0, cw_seed=None,
                 cw_left=None, cw_right=None, stride=16)[0] == 0


# ---- the plan -------------------------------------------------------------------------
LIMIT = hip_abi.EXPAND_ROWS_MAX_SUBTREE


def _aes_per_key(pl):
    S, walk = pl["S"], pl["walk"]
    return 2 ** walk * (walk + 2 * (2 ** S - 1) + 2 ** S)


# (K, depth, CUs) -> (S, walk): depth 0; items per key below, at and above 64;
# launches too small for 256 items per CU, lowered to enough items or to S = 0.
PLAN_TABLE = [
    ((1, 0, 256), (0, 0)), ((5, 0, 1), (0, 0)), ((1 << 20, 0, 256), (0, 0)),
    ((1 << 16, 11, 256), (6, 5)),         # 32 items per key
    ((1 << 12, 12, 256), (6, 6)),         # 64
    ((1 << 12, 15, 256), (6, 9)),         # 512
    ((96, 15, 256), (5, 10)),             # 96 * 2^9 < 65536 <= 96 * 2^10
    ((300, 4, 256), (0, 4)),              # too small at any depth
    ((64, 6, 256), (0, 6)), ((3, 12, 256), (0, 12)), ((1, 13, 256), (0, 13)),
    ((1, 23, 256), (6, 17)), ((1, 16, 256), (0, 16)), ((1, 17, 256), (1, 16)),
    (((1 << 31) - 1, 3, 256), (3, 0)), ((1, 8, 1), (0, 8)), ((2, 8, 1), (1, 7)),
    ((256, 6, 1), (6, 0)),
]


@pytest.mark.parametrize("args,want", PLAN_TABLE, ids=str)
def test_plan_table(args, want):
    K, depth, cus = args
    pl = hip_abi.expand_rows_plan(K, depth, cus)
    assert (pl["S"], pl["walk"]) == want
    assert pl["items_per_key"] == 2 ** pl["walk"] and pl["items"] == K * pl["items_per_key"]
    ideal = 2 * (2 ** depth - 1) + 2 ** depth
    assert _aes_per_key(pl) >= ideal
    if pl["walk"] == 0:
        assert _aes_per_key(pl) == ideal      # one item per key walks nothing twice


@pytest.mark.parametrize("num_cus", [1, 256])
@pytest.mark.parametrize("num_keys", [1, 70, 1 << 12, 1 << 20])
def test_plan_properties(num_keys, num_cus):
    assert hip_abi.expand_rows_plan(1 << 20, 23, 1)["S"] == LIMIT
    want = ITEMS_PER_CU * num_cus
    for depth in range(0, 24):
        pl = hip_abi.expand_rows_plan(num_keys, depth, num_cus)
        S, walk = pl["S"], pl["walk"]
        assert walk + S == depth and 0 <= S <= LIMIT and walk >= 0
        deepest = min(depth, LIMIT)
        if num_keys * 2 ** (depth - deepest) >= want:
            assert S == deepest, (depth, pl)
        else:
            assert S == 0 or pl["items"] >= want, (depth, pl)
            if S < deepest:
                assert num_keys * 2 ** (depth - (S + 1)) < want, (depth, pl)


def test_plan_bad_shapes():
    for args in ((0, 8, 256), (-1, 8, 256), (1 << 31, 8, 256), (1, -1, 256), (1, 24, 256),
                 (1, 8, 0)):
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.expand_rows_plan(*args)
        assert e.value.code == INVALID_ARGUMENT, args


# ---- dpf_hip_dot_buckets ------------------------------------------------------------
def _begin(*xs):
    return (ctypes.c_int64 * len(xs))(*xs)


def _fold(desc=None, null_desc=False, **over):
    """A call of dpf_hip_dot_buckets with dummy device pointers: rejected
    before anything dereferences them."""
    lib = hip_abi.load()
    d = desc if desc is not None else _desc(hip_abi.LEAF_INT, 64)
    a = dict(num_buckets=3, log_domain_size=8, record_words=4, bucket_begin=_begin(0, 1, 1, 5),
             num_keys=5, desc=_ptr(d), y=_P, y_stride=8 << 8, db=_P, out=_P, workspace=_P,
             workspace_bytes=1 << 30, stream=None)
    a.update(over)
    if null_desc:
        a["desc"] = None
    st = lib.dpf_hip_dot_buckets(*a.values())
    return st, lib.dpf_hip_last_error().decode()


@pytest.mark.parametrize("over", [
    dict(num_buckets=0), dict(num_buckets=(1 << 20) + 1), dict(log_domain_size=0),
    dict(log_domain_size=25), dict(record_words=0), dict(record_words=1025), dict(num_keys=-1),
    dict(num_keys=1 << 31), dict(null_desc=True), dict(bucket_begin=None),
    dict(bucket_begin=_begin(1, 1, 1, 5)), dict(bucket_begin=_begin(0, 2, 1, 5)),
    dict(bucket_begin=_begin(0, 1, 1, 4)), dict(bucket_begin=_begin(0, 1, 1, 6)),
    dict(y_stride=(8 << 8) - 16), dict(y_stride=(8 << 8) + 8), dict(y=None), dict(db=None),
    dict(out=None), dict(y=ctypes.c_void_p(_BASE + 8)), dict(workspace=ctypes.c_void_p(_BASE + 8)),
    dict(db=ctypes.c_void_p(_BASE + 4)), dict(out=ctypes.c_void_p(_BASE + 4)),
], ids=_stable_id)
def test_dot_buckets_argument_errors_are_invalid_argument(over):
    st, msg = _fold(**over)
    assert st == INVALID_ARGUMENT and msg


def test_dot_buckets_workspace_errors_name_the_bytes_needed():
    d = _desc(hip_abi.LEAF_INT, 64)
    need = hip_abi.dot_buckets_workspace_bytes(d, 4, 3, 5, 8)
    for over in (dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace_bytes=0)):
        st, msg = _fold(**over)
        assert st == RESOURCE_EXHAUSTED and str(need) in msg, over


def test_dot_buckets_two_faults_report_the_earlier_check():
    """Counts, NULL descriptor, value type, bucket_begin, the stride, the
    empty batch, NULL buffers, the workspace, alignment."""
    u32 = _desc(hip_abi.LEAF_INT, 32)
    # 1 before 2 and 3.
    assert "num_buckets" in _fold(num_buckets=0, null_desc=True)[1]
    assert "record_words" in _fold(record_words=0, desc=u32)[1]
    # 2 before 3 is one argument; 3 before 4: a bad type with a bad bucket_begin.
    assert _fold(desc=u32, bucket_begin=None)[0] == UNIMPLEMENTED
    # 4 before 5: a bad bucket_begin with a bad stride.
    assert "bucket_begin" in _fold(bucket_begin=_begin(0, 2, 1, 5), y_stride=8)[1]
    # 5 before 6: a bad stride is an error even without keys; so are 3 and 4.
    zeros = _begin(0, 0, 0, 0)
    st, msg = _fold(num_keys=0, bucket_begin=zeros, y_stride=8)
    assert st == INVALID_ARGUMENT and "y_stride_bytes" in msg
    assert _fold(num_keys=0, bucket_begin=zeros, desc=u32)[0] == UNIMPLEMENTED
    assert _fold(num_keys=0)[0] == INVALID_ARGUMENT          # bucket_begin ends at 5
    # 6 before 7 and 8: no keys return OK whatever the buffers.
    assert _fold(num_keys=0, bucket_begin=zeros, y=None, db=None, out=None, workspace=None)[0] == 0
    # 7 before 8: a NULL buffer with no workspace.
    st, msg = _fold(db=None, workspace=None)
    assert st == INVALID_ARGUMENT and "NULL" in msg
    # 8 before 9: a short workspace with a misaligned output.
    assert _fold(workspace_bytes=16, out=ctypes.c_void_p(_BASE + 4))[0] == RESOURCE_EXHAUSTED
    st, msg = _fold(out=ctypes.c_void_p(_BASE + 4))
    assert st == INVALID_ARGUMENT and "aligned" in msg


def test_workspace_bytes_is_monotone_and_bounded():
    d = _desc(hip_abi.LEAF_XOR, 64)
    f = hip_abi.dot_buckets_workspace_bytes
    base = f(d, 4, 96, 96, 16)
    assert base > 0 and base % 16 == 0
    prev = 0
    for K in (0, 1, 15, 16, 17, 96, 1000, 1 << 20, (1 << 31) - 1):
        cur = f(d, 4, 96, K, 16)
        assert cur >= prev and cur > 0, K
        prev = cur
    prev = 0
    for B in (1, 2, 96, 1 << 10, 1 << 20):
        cur = f(d, 4, B, 1 << 12, 16)
        assert cur >= prev
        prev = cur
    for W in (1, 64, 65, 1024):
        for n in (1, 12, 24):
            assert f(d, W, 96, 96, n) >= f(d, 1, 96, 96, 1)
    # Room for every tile (a bucket's keys in tiles of 16, none shared).
    assert f(d, 1, 6, 84, 1) >= 16 * (1 + 2 + 5 + 1)
    for args in ((0, 96, 96, 16), (1025, 96, 96, 16), (4, 0, 96, 16), (4, (1 << 20) + 1, 96, 16),
                 (4, 96, -1, 16), (4, 96, 1 << 31, 16), (4, 96, 96, 0), (4, 96, 96, 25)):
        assert f(d, *args) == -1, args
    assert f(_desc(hip_abi.LEAF_INT, 32), 4, 96, 96, 16) == -1
    assert f(None, 4, 96, 96, 16) == -1


# ---- the host API: every check before the device is touched, in order ---------
LEVEL_MSG = "`hierarchy_level` must be non-negative and less than parameters_.size()"
TYPE_MSG = "the bucketed database fold is implemented for uint64_t and XorWrapper<uint64_t> only"
DOMAIN_MSG = "the bucketed database fold takes a log_domain_size in [1, 24]"
WORDS_MSG = "`record_words` must be in [1, 1024]"
ENTRIES_MSG = "`bucket_begin` must hold between 2 and 2^20 + 1 entries"
START_MSG = "`bucket_begin` must start at 0"
ORDER_MSG = "`bucket_begin` must be nondecreasing"
END_MSG = "`bucket_begin` must end at the number of keys of the batch"
DB_MSG = "`db_bytes` must be num_buckets * 2^log_domain_size * record_words * 8"
NULL_MSG = "`device_db` and `device_out` must not be null"
OUT_MSG = "device output buffer too small"
BATCH_MSG = "key batch does not match this DistributedPointFunction"
ALIGN_MSG = "`device_db` and `device_out` must be aligned to 8 bytes"


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


def _raised(call):
    with pytest.raises(D.DpfStatusError) as e:
        call()
    return e.value.code, e.value.message


def test_evaluates_dot_buckets_on_device_by_type_and_level():
    for vt, n, want in ((("int", 64), 8, True), (("xor", 64), 8, True), (("int", 64), 1, True),
                        (("int", 64), 24, True), (("int", 64), 25, False), (("int", 64), 0, False),
                        (("int", 32), 8, False), (("xor", 128), 8, False),
                        (("intmodn", 64, MODN), 8, False),
                        (("tuple", [("int", 64), ("int", 64)]), 8, False)):
        dpf = make([(n, vt, 0)])
        assert dpf.evaluates_dot_buckets_on_device(0) is want, (vt, n)
        assert dpf.evaluates_dot_buckets_on_device(1) is False
        assert dpf.evaluates_dot_buckets_on_device(-1) is False
    two = make([(4, ("int", 32), 0), (10, ("int", 64), 0)])
    assert [two.evaluates_dot_buckets_on_device(h) for h in (0, 1)] == [False, True]


def test_host_checks_report_the_first_failing_one():
    """Level, value type (and its domain), record_words, bucket_begin, db_bytes,
    null pointers, out_bytes, the batch, alignment: every check fires, and two
    faults at once report the earlier."""
    K, n, B = 5, 6, 3
    N = 1 << n
    dpf = make([(n, ("int", 64), 0)])
    store = torch.zeros(B * N * 4 + 1, dtype=torch.int64)      # room for W = 4
    out = torch.zeros(K * 4, dtype=torch.int64)
    good = [0, 1, 1, 5]

    def db_of(w, b=B):
        return store[:b * N * w]

    def check(h=0, begin=good, db=None, w=1, o=out, keys=K, matches=True, obj=dpf):
        db = db_of(w) if db is None else db
        return _raised(lambda: obj.check_dot_buckets_args(keys, h, begin, db, w, o,
                                                          batch_matches=matches))

    for w in (1, 2, 4):
        dpf.check_dot_buckets_args(K, 0, good, db_of(w), w, out)      # the valid calls pass
    null = _Buffer(0, B * N * 8)
    # 1. the level, with every later fault present too.
    for h in (-1, 1):
        assert check(h=h, w=0, begin=[1], db=null, o=out[:1], matches=False) == \
            (INVALID_ARGUMENT, LEVEL_MSG)
    # 2. the value type before record_words, then the domain.
    for vt in (("int", 32), ("xor", 128), ("intmodn", 64, MODN)):
        assert check(obj=make([(n, vt, 0)]), w=0) == (UNIMPLEMENTED, TYPE_MSG)
    assert check(obj=make([(25, ("int", 64), 0)]), w=0) == (INVALID_ARGUMENT, DOMAIN_MSG)
    assert check(obj=make([(0, ("int", 64), 0)]), w=0) == (INVALID_ARGUMENT, DOMAIN_MSG)
    # 3. record_words before bucket_begin.
    for w in (0, -3, 1025):
        assert check(w=w, begin=[1], db=store[:5]) == (INVALID_ARGUMENT, WORDS_MSG)
    # 4. bucket_begin, each of its faults, before the database's size.
    for begin in ([], [0]):
        assert check(begin=begin, db=store[:5]) == (INVALID_ARGUMENT, ENTRIES_MSG)
    assert check(begin=[1, 1, 1, 5], db=store[:5]) == (INVALID_ARGUMENT, START_MSG)
    assert check(begin=[0, 2, 1, 5], db=store[:5]) == (INVALID_ARGUMENT, ORDER_MSG)
    assert check(begin=[0, 1, 1, 4], db=store[:5]) == (INVALID_ARGUMENT, END_MSG)
    assert check(begin=[0, 1, 1, 6], db=store[:5]) == (INVALID_ARGUMENT, END_MSG)
    assert check(begin=[0, 0, 0, 0], db=store[:5]) == (INVALID_ARGUMENT, END_MSG)
    # 5. the database's size is exact (it follows the buckets of bucket_begin),
    #    and comes before the null pointers.
    assert check(db=store[:B * N - 1], o=_Buffer(0, 8 * K)) == (INVALID_ARGUMENT, DB_MSG)
    assert check(db=store[:B * N + 1]) == (INVALID_ARGUMENT, DB_MSG)
    assert check(w=2, db=db_of(1)) == (INVALID_ARGUMENT, DB_MSG)
    assert check(begin=[0, 1, 5], db=db_of(1)) == (INVALID_ARGUMENT, DB_MSG)
    assert check(db=_Buffer(0, B * N * 8 - 8), o=out[:1]) == (INVALID_ARGUMENT, DB_MSG)
    # 6. null pointers before the output's size.
    assert check(db=null, o=out[:1]) == (INVALID_ARGUMENT, NULL_MSG)
    assert check(o=_Buffer(0, 8 * K)) == (INVALID_ARGUMENT, NULL_MSG)
    # 7. the output's size before the batch.
    assert check(o=out[:K - 1], matches=False) == (INVALID_ARGUMENT, OUT_MSG)
    assert check(w=4, o=out[:4 * K - 1]) == (INVALID_ARGUMENT, OUT_MSG)
    # 8. the batch before alignment.
    misaligned = _Buffer(store.data_ptr() + 4, B * N * 8)
    assert check(db=misaligned, matches=False) == (INVALID_ARGUMENT, BATCH_MSG)
    # 9. alignment.
    assert check(db=misaligned) == (INVALID_ARGUMENT, ALIGN_MSG)
    assert check(o=_Buffer(out.data_ptr() + 4, 8 * K)) == (INVALID_ARGUMENT, ALIGN_MSG)
    # An empty batch still has its arguments checked.
    assert check(keys=0, begin=[0, 0, 0, 0], w=0) == (INVALID_ARGUMENT, WORDS_MSG)
    assert check(keys=0) == (INVALID_ARGUMENT, END_MSG)
    dpf.check_dot_buckets_args(0, 0, [0, 0, 0, 0], db_of(1), 1, out[:1])
