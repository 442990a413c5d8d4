"""Batched private table lookup (dpf_hip_lookup_batch,
EvaluateLookupBatch[ToDevice]) as far as it can be checked without a GPU: the
C ABI's declarations, the supported types, the argument checks and their order,
the launch plan and the order of the host API's checks."""
import ctypes
import re

import pytest
import torch

from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from test_key_batch_cpu import make

INVALID_ARGUMENT, UNIMPLEMENTED = 3, 12
SYMBOLS = ("dpf_hip_lookup_batch", "dpf_hip_lookup_supported", "dpf_hip_lookup_plan")
ITEMS_PER_CU = 256
MODN = 18446744073709551557


def _desc(kind, bits):
    return hip_abi.value_desc([(kind, bits, 0)], True, 128 // bits, 1)


def _limit(w):
    """The deepest subtree the kernel's stack allows for this table width: what
    the plan gives a launch with items to spare."""
    return hip_abi.lookup_plan(1 << 20, 39, w, 1)["S"]


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
@pytest.mark.parametrize("w", [1, 2, 4])
def test_supported(kind, w):
    assert hip_abi.lookup_supported(_desc(kind, 64), w)


def test_unsupported_types_widths_and_null():
    for kind in (hip_abi.LEAF_INT, hip_abi.LEAF_XOR):
        for bits in (8, 16, 32, 128):
            assert not hip_abi.lookup_supported(_desc(kind, bits), 1), (kind, bits)
        for w in (3, 0, -1, 5, 8, 1024, 1025):
            assert not hip_abi.lookup_supported(_desc(kind, 64), w), w
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    pair64 = hip_abi.value_desc([(hip_abi.LEAF_INT, 64, 0)] * 2, True, 1, 1)
    for d in (modn, pair, pair64):
        assert not hip_abi.lookup_supported(d, 1)
    assert not hip_abi.lookup_supported(None, 1)


_RAW = (ctypes.c_uint64 * 66)()
_BASE = (ctypes.addressof(_RAW) + 15) & ~15     # a 16-byte aligned dummy, never read


def _abi_args(desc=None, null_desc=False, **over):
    """A call of dpf_hip_lookup_batch whose pointers are non-null, 16-byte
    aligned dummies: it must be rejected before anything dereferences them.
    `desc`: the value descriptor (default uint64_t); null_desc: a NULL one."""
    p = ctypes.c_void_p(_BASE)
    key = hip_abi.aes_key(0)
    kp = ctypes.cast(ctypes.pointer(key), ctypes.c_void_p)
    d = desc if desc is not None else _desc(hip_abi.LEAF_INT, 64)
    a = dict(num_keys=2, num_levels=7, cw_stride=7, log_domain_size=8, key_seed=p, party=p,
             cw_seed=p, cw_left=p, cw_right=p, kl=kp, kr=kp, kv=kp,
             desc=ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), vcw=p, offsets=p, table=p,
             table_words=1, out=p, stream=None)
    a.update(over)
    if null_desc:
        a["desc"] = None
    return list(a.values()), (key, d)


def _call(**over):
    lib = hip_abi.load()
    args, keep = _abi_args(**over)
    st = lib.dpf_hip_lookup_batch(*args)
    return st, lib.dpf_hip_last_error().decode()


@pytest.mark.parametrize("over", [
    dict(num_keys=-1), dict(num_keys=1 << 31), dict(log_domain_size=0, num_levels=-1),
    dict(log_domain_size=41, num_levels=40), dict(num_levels=8), dict(num_levels=6),
    dict(kl=None), dict(kr=None), dict(kv=None), dict(null_desc=True),
    dict(table_words=0), dict(table_words=-2), dict(table_words=1025),
    dict(cw_stride=6), dict(key_seed=None), dict(party=None), dict(cw_seed=None),
    dict(cw_left=None), dict(cw_right=None), dict(vcw=None), dict(offsets=None),
    dict(table=None), dict(out=None),
], ids=str)
def test_argument_errors_are_invalid_argument(over):
    st, msg = _call(**over)
    assert st == INVALID_ARGUMENT and msg


def test_misaligned_buffers_are_invalid_argument():
    by8, by4 = ctypes.c_void_p(_BASE + 8), ctypes.c_void_p(_BASE + 4)
    for over in (dict(table=by4), dict(out=by4), dict(offsets=by4),
                 dict(table=by8, table_words=2), dict(table=by8, table_words=4)):
        st, msg = _call(**over)
        assert st == INVALID_ARGUMENT and "aligned" in msg, over


def test_unsupported_type_and_width_are_unimplemented():
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    for d in (modn, pair, _desc(hip_abi.LEAF_INT, 32), _desc(hip_abi.LEAF_XOR, 128)):
        assert _call(desc=d)[0] == UNIMPLEMENTED
    for w in (3, 5, 8, 1024):
        assert _call(table_words=w)[0] == UNIMPLEMENTED, w


def test_two_faults_report_the_earlier_check():
    """The documented order: counts and domain, NULL descriptor or AES key,
    value type, table_words' range, table_words' set, cw_stride, the empty
    batch, NULL arrays, alignment."""
    u32 = _desc(hip_abi.LEAF_INT, 32)
    # 1 before 2, 3, 4: a bad count with a NULL key, a bad type, a bad width.
    assert _call(num_keys=-1, kl=None, desc=u32, table_words=0)[0] == INVALID_ARGUMENT
    assert "num_keys" in _call(num_keys=-1, desc=u32)[1]
    assert "log_domain_size" in _call(log_domain_size=0, num_levels=-1, desc=u32)[1]
    # 2 before 3: a NULL AES key with an unsupported type.
    assert _call(kl=None, desc=u32)[0] == INVALID_ARGUMENT
    # 3 before 4: an unsupported type with table_words out of range.
    assert _call(desc=u32, table_words=0)[0] == UNIMPLEMENTED
    # 4 before 5 is one argument; 5 before 6: an unsupported width with a short stride.
    assert _call(table_words=1025, cw_stride=0)[0] == INVALID_ARGUMENT
    assert "table_words" in _call(table_words=1025, cw_stride=0)[1]
    assert _call(table_words=3, cw_stride=0)[0] == UNIMPLEMENTED
    # 6 before 7: a short stride is an error even for an empty batch.
    assert _call(num_keys=0, cw_stride=6)[0] == INVALID_ARGUMENT
    # 3 and 5 before 7: so are an unsupported type and width.
    assert _call(num_keys=0, desc=u32)[0] == UNIMPLEMENTED
    assert _call(num_keys=0, table_words=3)[0] == UNIMPLEMENTED
    # 7 before 8: an empty batch returns OK whatever the arrays.
    assert _call(num_keys=0, key_seed=None, party=None, table=None, out=None)[0] == 0
    # 8 before 9: a NULL array with a misaligned table.
    st, msg = _call(out=None, table=ctypes.c_void_p(12))
    assert st == INVALID_ARGUMENT and "NULL" in msg


def test_no_tree_needs_no_correction_words():
    """n = 1: the key's root is the only node, and NULL correction words pass
    the checks (the empty batch keeps the call off the device)."""
    assert _call(num_keys=0, log_domain_size=1, num_levels=0, cw_stride=0, cw_seed=None,
                 cw_left=None, cw_right=None)[0] == 0


@pytest.mark.parametrize("num_cus", [1, 256])
@pytest.mark.parametrize("w", [1, 2, 4])
@pytest.mark.parametrize("num_keys", [1, 70, 1 << 12, 1 << 20])
def test_plan_properties(num_keys, w, num_cus):
    limit = _limit(w)
    assert 1 <= limit <= 12
    want = ITEMS_PER_CU * num_cus
    for depth in range(0, 24):
        pl = hip_abi.lookup_plan(num_keys, depth, w, num_cus)
        S, walk = pl["S"], pl["walk"]
        assert walk + S == depth and S >= 0 and walk >= 0
        assert pl["items_per_key"] == 2 ** walk
        assert pl["items"] == num_keys * pl["items_per_key"]
        assert S <= limit
        deepest = min(depth, limit)
        if num_keys * 2 ** (depth - deepest) >= want:
            assert S == deepest, (depth, pl)
        else:
            # Lowered (a tree of depth 0 has nothing to lower), down to enough
            # items or to 0, and no further than needed: S + 1 would have left
            # the launch short of items.
            assert S < deepest or deepest == 0, (depth, pl)
            assert S == 0 or pl["items"] >= want, (depth, pl)
            if S < deepest:
                assert num_keys * 2 ** (depth - (S + 1)) < want, (depth, pl)


def test_plan_limits_and_bad_shapes():
    # The limits the header documents, from the compiler's register report.
    assert (_limit(1), _limit(2), _limit(4)) == (5, 5, 4)
    for args in ((0, 8, 1, 256), (-1, 8, 1, 256), (1 << 31, 8, 1, 256), (1, -1, 1, 256),
                 (1, 40, 1, 256), (1, 8, 3, 256), (1, 8, 0, 256), (1, 8, 1, 0)):
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.lookup_plan(*args)
        assert e.value.code == INVALID_ARGUMENT, args


# ---- the host API: every check before the device is touched, in order ---------
LEVEL_MSG = "`hierarchy_level` must be non-negative and less than parameters_.size()"
TYPE_MSG = "the table lookup is implemented for uint64_t and XorWrapper<uint64_t> only"
DOMAIN_MSG = "the table lookup takes a log_domain_size in [1, 40]"
WORDS_MSG = "`table_words` must be in [1, 1024]"
WIDTH_MSG = "the table lookup is implemented for table_words 1, 2 and 4 only"
TABLE_MSG = "`table_bytes` must be 2^log_domain_size * table_words * 8"
NULL_MSG = "`device_offsets`, `device_table` and `device_out` must not be null"
OUT_MSG = "device output buffer too small"
BATCH_MSG = "key batch does not match this DistributedPointFunction"


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


def test_evaluates_lookup_on_device_by_type_and_level():
    for vt, n, want in ((("int", 64), 8, True), (("xor", 64), 8, True), (("int", 64), 1, True),
                        (("int", 64), 40, True), (("int", 64), 41, False), (("int", 64), 0, False),
                        (("int", 32), 8, False), (("xor", 128), 8, False),
                        (("intmodn", 64, MODN), 8, False),
                        (("tuple", [("int", 64), ("int", 64)]), 8, False)):
        dpf = make([(n, vt, 0)])
        assert dpf.evaluates_lookup_on_device(0) is want, (vt, n)
        assert dpf.evaluates_lookup_on_device(1) is False
        assert dpf.evaluates_lookup_on_device(-1) is False
    two = make([(4, ("int", 32), 0), (10, ("int", 64), 0)])
    assert [two.evaluates_lookup_on_device(h) for h in (0, 1)] == [False, True]


def test_host_checks_report_the_first_failing_one():
    """Level, value type (and its domain), table_words, table_bytes, null
    pointers, out_bytes, the batch, alignment: two faults at once report the
    earlier."""
    K, n = 3, 8
    dpf = make([(n, ("int", 64), 0)])
    table = torch.zeros((1 << n) * 4, dtype=torch.int64)       # room for W = 4
    offsets = torch.zeros(K, dtype=torch.int64)
    out = torch.zeros(K * 4, dtype=torch.int64)
    null = _Buffer(0, (1 << n) * 8)

    def check(h=0, off=offsets, tab=None, w=1, o=out, keys=K, matches=True, obj=dpf):
        tab = table[:(1 << n) * w] if tab is None else tab
        return _raised(lambda: obj.check_lookup_args(keys, h, off, tab, w, o,
                                                     batch_matches=matches))

    dpf.check_lookup_args(K, 0, offsets, table[:1 << n], 1, out)   # the valid call passes
    for w in (1, 2, 4):
        dpf.check_lookup_args(K, 0, offsets, table[:(1 << n) * w], w, out)
    # The level, with every later fault present too.
    for h in (-1, 1):
        assert check(h=h, w=0, tab=null, o=out[:1], matches=False) == (INVALID_ARGUMENT, LEVEL_MSG)
    # The value type before table_words.
    for vt in (("int", 32), ("xor", 128), ("intmodn", 64, MODN)):
        other = make([(n, vt, 0)])
        assert check(obj=other, w=0, tab=null) == (UNIMPLEMENTED, TYPE_MSG)
    assert check(obj=make([(41, ("int", 64), 0)]), w=0) == (INVALID_ARGUMENT, DOMAIN_MSG)
    assert check(obj=make([(0, ("int", 64), 0)]), w=3) == (INVALID_ARGUMENT, DOMAIN_MSG)
    # table_words: its range (3), then its set (12), before the table's size.
    for w in (0, -3, 1025):
        assert check(w=w, tab=table[:5]) == (INVALID_ARGUMENT, WORDS_MSG)
    for w in (3, 8, 1024):
        assert check(w=w, tab=table[:5]) == (UNIMPLEMENTED, WIDTH_MSG)
    # The table's size is exact, and comes before the null pointers.
    assert check(tab=table[:(1 << n) - 1], off=_Buffer(0, 8)) == (INVALID_ARGUMENT, TABLE_MSG)
    assert check(tab=table[:(1 << n) + 1]) == (INVALID_ARGUMENT, TABLE_MSG)
    assert check(w=2, tab=table[:1 << n]) == (INVALID_ARGUMENT, TABLE_MSG)
    assert check(tab=_Buffer(0, (1 << n) * 8 - 8), o=out[:1]) == (INVALID_ARGUMENT, TABLE_MSG)
    # Null pointers before the output's size.
    assert check(tab=null, o=out[:1]) == (INVALID_ARGUMENT, NULL_MSG)
    assert check(off=_Buffer(0, 8 * K), o=out[:1]) == (INVALID_ARGUMENT, NULL_MSG)
    assert check(o=_Buffer(0, 8 * K)) == (INVALID_ARGUMENT, NULL_MSG)
    # The output's size before the batch.
    assert check(o=out[:K - 1], matches=False) == (INVALID_ARGUMENT, OUT_MSG)
    assert check(w=4, o=out[:4 * K - 1]) == (INVALID_ARGUMENT, OUT_MSG)
    # The batch before alignment.
    misaligned = _Buffer(table.data_ptr() + 4, (1 << n) * 8)
    assert check(tab=misaligned, matches=False) == (INVALID_ARGUMENT, BATCH_MSG)
    code, msg = check(tab=misaligned)
    assert code == INVALID_ARGUMENT and "aligned" in msg
    code, msg = check(w=2, tab=_Buffer(table.data_ptr() + 8, (1 << n) * 16))
    assert code == INVALID_ARGUMENT and "aligned" in msg
    # An empty batch still has its arguments checked.
    assert check(keys=0, w=3) == (UNIMPLEMENTED, WIDTH_MSG)
    dpf.check_lookup_args(0, 0, offsets, table[:1 << n], 1, out[:0].new_zeros(1))
