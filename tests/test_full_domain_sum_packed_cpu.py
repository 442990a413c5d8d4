"""The packed full-domain sum (dpf_hip_expand_sum_packed,
EvaluateFullDomainSumPacked[ToDevice], histogram.fold / reconstruct_packed) as
far as it can be checked without a GPU: the C ABI's declarations, the supported
types, the argument checks and their order in both layers, the shapes the host
takes, histogram.reconstruct_packed, and a NumPy model of the kernel's
element-wise word add and of the butterfly with it."""
import ctypes
import re

import numpy as np
import pytest
import torch

import packed_sum_model as M
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import histogram as HG
from test_key_batch_cpu import make

INVALID_ARGUMENT, RESOURCE_EXHAUSTED, UNIMPLEMENTED = 3, 8, 12
SYMBOLS = ("dpf_hip_expand_sum_packed", "dpf_hip_expand_sum_packed_supported")
MODN = 18446744073709551557
NINE = [("int", 8), ("int", 16), ("int", 32), ("int", 64),
        ("xor", 8), ("xor", 16), ("xor", 32), ("xor", 64), ("xor", 128)]
KIND = {"int": hip_abi.LEAF_INT, "xor": hip_abi.LEAF_XOR}


def _desc(kind, bits):
    return hip_abi.value_desc([(kind, bits, 0)], True, 128 // bits, 1)


def _log2e(bits):
    return (128 // bits).bit_length() - 1


# ---- exports --------------------------------------------------------------------
def test_header_and_abi_declare_the_entry_points():
    names = hip_abi.header_functions()
    lib = hip_abi.load()
    src = open(hip_abi.__file__).read()
    for f in SYMBOLS:
        assert f in names
        assert hasattr(lib, f), f
        assert re.search(r'"%s"' % f, src), f
        assert getattr(lib, f).argtypes is not None
    assert lib.dpf_hip_abi_version() == 2
    assert "#define DPF_HIP_ABI_VERSION 2\n" in open(hip_abi.HEADER).read()


def test_supported_types():
    for kind, bits in NINE:
        assert hip_abi.expand_sum_packed_supported(_desc(KIND[kind], bits)), (kind, bits)
        # The earlier call says what it said.
        assert hip_abi.expand_sum_supported(_desc(KIND[kind], bits)) is (bits == 64)
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN)], False, 1, 1)
    modn32 = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 32, 4294967291)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    pair64 = hip_abi.value_desc([(hip_abi.LEAF_INT, 64, 0)] * 2, True, 1, 1)
    for d in (_desc(hip_abi.LEAF_INT, 128), modn, modn32, pair, pair64):
        assert not hip_abi.expand_sum_packed_supported(d)
        assert not hip_abi.expand_sum_supported(d)
    assert not hip_abi.expand_sum_packed_supported(None)
    assert not hip_abi.expand_sum_supported(None)


# ---- dpf_hip_expand_sum_packed: every check before the device is touched -----------
_RAW = (ctypes.c_uint64 * 66)()
_BASE = (ctypes.addressof(_RAW) + 15) & ~15     # a 16-byte aligned dummy, never read


def _abi_args(desc=None, null_desc=False, **over):
    """A call whose pointers are non-null, 16-byte aligned dummies: it must be
    rejected before anything dereferences them.  uint32_t, n = 8: 6 levels."""
    p = ctypes.c_void_p(_BASE)
    key = hip_abi.aes_key(0)
    kp = ctypes.cast(ctypes.pointer(key), ctypes.c_void_p)
    d = desc if desc is not None else _desc(hip_abi.LEAF_INT, 32)
    a = dict(num_keys=2, num_levels=6, cw_stride=6, log_domain_size=8, key_seed=p, party=p,
             cw_seed=p, cw_left=p, cw_right=p, kl=kp, kr=kp, kv=kp,
             desc=ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), vcw=p, workspace=p,
             workspace_bytes=hip_abi.expand_sum_workspace_bytes(2, 6), out=p,
             out_bytes=(1 << 8) * 4, accumulate=1, stream=None)
    a.update(over)
    if null_desc:
        a["desc"] = None
    return list(a.values()), (key, d)


def _call(**over):
    lib = hip_abi.load()
    args, keep = _abi_args(**over)
    st = lib.dpf_hip_expand_sum_packed(*args)
    return st, lib.dpf_hip_last_error().decode()


@pytest.mark.parametrize("over", [
    # 1. sizes
    dict(num_keys=-1), dict(num_keys=1 << 31), dict(log_domain_size=-1, num_levels=-3),
    dict(log_domain_size=31, num_levels=29),
    # 2. desc and AES keys
    dict(kl=None), dict(kr=None), dict(kv=None), dict(null_desc=True),
    # 3a. the tree's depth: n - log2 E, not the 64-bit call's n - 1
    dict(num_levels=7), dict(num_levels=5), dict(log_domain_size=1, num_levels=-1),
    dict(log_domain_size=1, num_levels=0),
    # 4. cw_stride, 5. out and its size
    dict(cw_stride=5), dict(out=None), dict(out_bytes=(1 << 8) * 4 - 1), dict(out_bytes=0),
    # 7. key arrays
    dict(key_seed=None), dict(party=None), dict(cw_seed=None), dict(cw_left=None),
    dict(cw_right=None), dict(vcw=None),
], ids=str)
def test_argument_errors_are_invalid_argument(over):
    st, msg = _call(**over)
    assert st == INVALID_ARGUMENT and msg


@pytest.mark.parametrize("kind,bits", NINE, ids=str)
def test_num_levels_is_the_domain_less_the_elements_of_a_block(kind, bits):
    """n = 8 of every type: n - log2 E levels pass the checks (the call stops
    at the short workspace, before the device), one more or fewer do not, and
    `out` is N * B / 8 bytes."""
    d = _desc(KIND[kind], bits)
    levels = 8 - _log2e(bits)
    good = dict(desc=d, num_levels=levels, cw_stride=levels, out_bytes=(1 << 8) * bits // 8,
                workspace_bytes=0)
    assert _call(**good)[0] == RESOURCE_EXHAUSTED
    for off in (-1, 1):
        st, msg = _call(**dict(good, num_levels=levels + off, cw_stride=levels + 1))
        assert st == INVALID_ARGUMENT and "at least one full leaf block" in msg
    st, msg = _call(**dict(good, out_bytes=(1 << 8) * bits // 8 - 1))
    assert st == INVALID_ARGUMENT and "`out`" in msg
    # The smallest domain of the type: one leaf block, no tree.
    small = dict(desc=d, log_domain_size=_log2e(bits), num_levels=0, cw_stride=0, out_bytes=16,
                 cw_seed=None, cw_left=None, cw_right=None, workspace_bytes=0)
    assert _call(**small)[0] == RESOURCE_EXHAUSTED
    if bits < 128:
        st, msg = _call(**dict(small, log_domain_size=_log2e(bits) - 1, num_levels=-1))
        assert st == INVALID_ARGUMENT and "at least one full leaf block" in msg


def test_the_stack_bounds_the_tree_at_29_levels():
    x128 = _desc(hip_abi.LEAF_XOR, 128)
    ok = dict(desc=x128, log_domain_size=29, num_levels=29, cw_stride=29, out_bytes=16 << 29,
              workspace_bytes=0)
    assert _call(**ok)[0] == RESOURCE_EXHAUSTED
    st, msg = _call(**dict(ok, log_domain_size=30, num_levels=30, cw_stride=30,
                           out_bytes=16 << 30))
    assert st == INVALID_ARGUMENT and "[0, 29]" in msg
    u32 = dict(log_domain_size=30, num_levels=28, cw_stride=28, out_bytes=4 << 30,
               workspace_bytes=0)
    assert _call(**u32)[0] == RESOURCE_EXHAUSTED


def test_unsupported_types_are_unimplemented():
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    for d in (_desc(hip_abi.LEAF_INT, 128), pair, modn):
        st, msg = _call(desc=d)
        assert st == UNIMPLEMENTED
        assert "uint8_t" in msg and "uint128" in msg and "at least one full leaf block" in msg


def test_empty_batch_returns_ok_without_a_launch():
    """accumulate set: `out` is left as it is, and nothing touches a device."""
    assert _call(num_keys=0)[0] == 0
    assert _call(num_keys=0, key_seed=None, party=None, vcw=None, workspace=None,
                 workspace_bytes=0)[0] == 0


def test_workspace_and_alignment():
    need = hip_abi.expand_sum_workspace_bytes(2, 6)
    for over in (dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace=None)):
        st, msg = _call(**over)
        assert st == RESOURCE_EXHAUSTED and str(need) in msg, over
    for over in (dict(out=ctypes.c_void_p(_BASE + 8)), dict(workspace=ctypes.c_void_p(_BASE + 8)),
                 dict(out=ctypes.c_void_p(_BASE + 4))):
        st, msg = _call(**over)
        assert st == INVALID_ARGUMENT and "aligned" in msg, over


def test_two_faults_report_the_earlier_check():
    i128 = _desc(hip_abi.LEAF_INT, 128)
    by8 = ctypes.c_void_p(_BASE + 8)
    # 1 before 2, 3: a bad count with a NULL key and a bad type.
    assert "num_keys" in _call(num_keys=-1, kl=None, desc=i128)[1]
    assert "log_domain_size" in _call(log_domain_size=31, null_desc=True)[1]
    # 2 before 3: a NULL AES key with an unsupported type.
    assert _call(kl=None, desc=i128)[0] == INVALID_ARGUMENT
    # 3 before 3a, 4 and 5.
    assert _call(desc=i128, num_levels=3)[0] == UNIMPLEMENTED
    assert _call(desc=i128, cw_stride=0)[0] == UNIMPLEMENTED
    assert _call(desc=i128, out=None)[0] == UNIMPLEMENTED
    # 3a before 4: a wrong depth with a short stride.
    assert "num_levels" in _call(num_levels=7, cw_stride=0)[1]
    # 4 before 5: a short stride with a NULL out; NULL before the size.
    assert "cw_stride" in _call(cw_stride=0, out=None)[1]
    assert "NULL" in _call(out=None, out_bytes=0)[1]
    # 3, 4, 5 before 6: an empty batch still has them checked.
    assert _call(num_keys=0, desc=i128)[0] == UNIMPLEMENTED
    assert _call(num_keys=0, cw_stride=5)[0] == INVALID_ARGUMENT
    assert _call(num_keys=0, out=None)[0] == INVALID_ARGUMENT
    assert _call(num_keys=0, out_bytes=8)[0] == INVALID_ARGUMENT
    # 6 before 7, 8, 9: an empty batch returns OK whatever the arrays.
    assert _call(num_keys=0, key_seed=None, workspace=None, out=by8)[0] == 0
    # 7 before 8: a NULL array with a short workspace.
    st, msg = _call(party=None, workspace_bytes=0)
    assert st == INVALID_ARGUMENT and "NULL" in msg
    # 8 before 9: a short workspace with a misaligned out.
    assert _call(workspace_bytes=0, out=by8)[0] == RESOURCE_EXHAUSTED


# ---- the host API --------------------------------------------------------------------
LEVEL_MSG = "`hierarchy_level` must be non-negative and less than parameters_.size()"
OLD_TYPE_MSG = "the full-domain sum is implemented for uint64_t and XorWrapper<uint64_t> only"
NULL_MSG = "`device_out` must not be null"
OUT_MSG = "device output buffer too small"
BATCH_MSG = "key batch does not match this DistributedPointFunction"
ALIGN_MSG = "`device_out` must be aligned to 16 bytes"


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


@pytest.mark.parametrize("vt,n,want", [
    (("int", 8), 3, False),      # below a leaf block
    (("int", 8), 4, True), (("int", 32), 2, True), (("int", 32), 30, True),
    (("int", 32), 31, False), (("xor", 128), 29, True), (("xor", 128), 30, False),
    (("xor", 128), 0, True), (("int", 16), 2, False), (("int", 64), 0, False),
    (("int", 64), 1, True), (("int", 64), 30, True), (("xor", 8), 20, True),
    (("int", 128), 8, False), (("intmodn", 64, MODN), 8, False),
    (("tuple", [("int", 32), ("int", 32)]), 8, False),
], ids=str)
def test_evaluates_full_domain_sum_packed_on_device(vt, n, want):
    dpf = make([(n, vt, 0)])
    assert dpf.evaluates_full_domain_sum_packed_on_device(0) is want
    assert dpf.evaluates_full_domain_sum_packed_on_device(1) is False
    assert dpf.evaluates_full_domain_sum_packed_on_device(-1) is False


def test_hierarchy_levels_need_full_leaf_blocks():
    """[(3, u8), (4, u8)]: level 0 is below a block, and level 1's tree level
    is forced past it, so its blocks are half used.  [(6, u32), (11, xor16)]:
    both levels sit at n - log2 E."""
    two = make([(3, ("int", 8), 0), (4, ("int", 8), 0)])
    assert [two.evaluates_full_domain_sum_packed_on_device(h) for h in (0, 1)] == [False, False]
    two = make([(6, ("int", 32), 0), (11, ("xor", 16), 0)])
    assert two.hierarchy_to_tree() == [4, 8]
    assert [two.evaluates_full_domain_sum_packed_on_device(h) for h in (0, 1)] == [True, True]
    # The earlier call still takes 64 bits alone.
    assert [two.evaluates_full_domain_sum_on_device(h) for h in (0, 1)] == [False, False]


def test_host_checks_report_the_first_failing_one():
    """Level, type and shape, null pointer, out_bytes, the batch, alignment:
    each tripped alone, and two faults at once report the earlier."""
    K, n = 3, 8
    N = 1 << n
    dpf = make([(n, ("int", 16), 0)])
    raw = torch.zeros(N + 8, dtype=torch.int16)
    shift = (-raw.data_ptr() % 16) // 2
    out = raw[shift:shift + N]                 # 16-byte aligned, N elements
    assert out.data_ptr() % 16 == 0
    null = _Buffer(0, N * 2)
    misaligned = _Buffer(out.data_ptr() + 8, N * 2)

    def check(h=0, o=out, keys=K, matches=True, obj=dpf):
        return _raised(lambda: obj.check_full_domain_sum_packed_args(keys, h, o,
                                                                      batch_matches=matches))

    def unimplemented(result):
        code, msg = result
        return (code == UNIMPLEMENTED and "uint8_t" in msg and "uint128" in msg
                and "at least one full leaf block" in msg)

    dpf.check_full_domain_sum_packed_args(K, 0, out)       # the valid call passes
    dpf.check_full_domain_sum_packed_args(0, 0, out)       # and an empty batch
    # Each check alone.
    assert check(h=1) == (INVALID_ARGUMENT, LEVEL_MSG)
    for vt, m in ((("int", 128), n), (("intmodn", 64, MODN), n), (("int", 8), 3),
                  (("int", 32), 31), (("xor", 128), 30),
                  (("tuple", [("int", 32), ("int", 32)]), n)):
        assert unimplemented(check(obj=make([(m, vt, 0)]), o=_Buffer(out.data_ptr(), 1 << 40)))
    assert check(o=null) == (INVALID_ARGUMENT, NULL_MSG)
    assert check(o=out[:N - 1]) == (INVALID_ARGUMENT, OUT_MSG)
    assert check(keys=-1) == (INVALID_ARGUMENT, OUT_MSG)
    assert check(matches=False) == (INVALID_ARGUMENT, BATCH_MSG)
    assert check(o=misaligned) == (INVALID_ARGUMENT, ALIGN_MSG)
    # The level, with every later fault present too.
    for h in (-1, 1):
        assert check(h=h, o=_Buffer(0, 8), matches=False) == (INVALID_ARGUMENT, LEVEL_MSG)
    # Type and shape before the null pointer.
    assert unimplemented(check(obj=make([(n, ("int", 128), 0)]), o=_Buffer(0, 8), matches=False))
    assert unimplemented(check(obj=make([(3, ("int", 8), 0), (4, ("int", 8), 0)]), h=1, o=null))
    # The null pointer before the size, the size before the batch, the batch before alignment.
    assert check(o=_Buffer(0, 8), matches=False) == (INVALID_ARGUMENT, NULL_MSG)
    assert check(o=_Buffer(out.data_ptr() + 8, N * 2 - 8), matches=False) == \
        (INVALID_ARGUMENT, OUT_MSG)
    assert check(o=misaligned, matches=False) == (INVALID_ARGUMENT, BATCH_MSG)
    assert check(keys=0, o=null) == (INVALID_ARGUMENT, NULL_MSG)
    dpf.check_full_domain_sum_packed_args(K, 0, _Buffer(out.data_ptr(), N * 2 + 64))
    # The size is the packed one: N bytes of uint8, 16 N of XorWrapper<uint128>.
    for vt, size in ((("int", 8), 1), (("xor", 32), 4), (("int", 64), 8), (("xor", 128), 16)):
        obj = make([(n, vt, 0)])
        obj.check_full_domain_sum_packed_args(K, 0, _Buffer(out.data_ptr(), N * size))
        assert check(obj=obj, o=_Buffer(out.data_ptr(), N * size - 1)) == \
            (INVALID_ARGUMENT, OUT_MSG)


def test_the_earlier_call_refuses_what_it_refused():
    dpf = make([(8, ("int", 32), 0)])
    out = _Buffer(_BASE, 1 << 20)
    assert _raised(lambda: dpf.check_full_domain_sum_args(3, 0, out)) == \
        (UNIMPLEMENTED, OLD_TYPE_MSG)
    assert dpf.evaluates_full_domain_sum_on_device(0) is False


# ---- histogram.reconstruct_packed ----------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16, 32, 64])
def test_reconstruct_packed_wraps_at_the_element(bits):
    top = (1 << bits) - 1
    dt = M.DTYPE[bits]
    a = np.array([1, top, 5, 1 << (bits - 1), 0, top], dtype=dt)
    b = np.array([2, 1, top - 4, 1 << (bits - 1), 0, top], dtype=dt)
    got = HG.reconstruct_packed(a, b, bits, False)
    assert got.dtype == dt
    np.testing.assert_array_equal(got, np.array([3, 0, 0, 0, 0, top - 1], dtype=dt))
    np.testing.assert_array_equal(HG.reconstruct_packed(a, b, bits, True),
                                  np.array([3, top - 1, 5 ^ (top - 4), 0, 0, 0], dtype=dt))
    # Signed storage (torch has no unsigned arithmetic above 8 bits) is taken as its bits.
    signed = {8: np.int8, 16: np.int16, 32: np.int32, 64: np.int64}[bits]
    tb = torch.from_numpy(b.view(signed)) if bits > 8 else torch.from_numpy(b)
    np.testing.assert_array_equal(HG.reconstruct_packed(a.view(signed), tb, bits, False), got)


def test_reconstruct_packed_128_bits_is_xor_alone():
    a = np.array([[1, 2], [(1 << 64) - 1, 7]], dtype=np.uint64)
    b = np.array([[3, 2], [1, 1 << 63]], dtype=np.uint64)
    got = HG.reconstruct_packed(a.view(np.int64), b, 128, True)
    assert got.shape == (2, 2) and got.dtype == np.uint64
    np.testing.assert_array_equal(got, a ^ b)
    with pytest.raises(ValueError):
        HG.reconstruct_packed(a, b, 128, False)
    with pytest.raises(ValueError):
        HG.reconstruct_packed(a, b, 24, True)


# ---- the word-level element add and the butterfly with it ------------------------------
def test_byte_add_is_exhaustive_at_every_byte_position():
    """Every pair of bytes at each of the 8 positions of a word, the other
    seven bytes all ones (every carry that could leak would show)."""
    x = np.arange(256, dtype=np.uint64)
    a, b = np.meshgrid(x, x, indexing="ij")
    for pos in range(8):
        rest = np.uint64(M.M64 ^ (0xFF << (8 * pos)))
        wa = (a << np.uint64(8 * pos)) | rest
        wb = (b << np.uint64(8 * pos)) | rest
        np.testing.assert_array_equal(M.word_add(wa, wb, 8), M.element_add(wa, wb, 8))
        wb = b << np.uint64(8 * pos)
        np.testing.assert_array_equal(M.word_add(wa, wb, 8), M.element_add(wa, wb, 8))


@pytest.mark.parametrize("bits", [8, 16, 32, 64])
def test_word_add_equals_the_element_add_on_random_words(bits):
    rng = np.random.default_rng(bits)
    a = rng.integers(0, 1 << 64, size=20000, dtype=np.uint64)
    b = rng.integers(0, 1 << 64, size=20000, dtype=np.uint64)
    # Elements at their edges as well: all ones, a lone top bit, zero.
    edges = np.array([M.M64, M.top_bits(bits), 0, M.M64 ^ M.top_bits(bits), 1], dtype=np.uint64)
    a[:25] = np.repeat(edges, 5)
    b[:25] = np.tile(edges, 5)
    np.testing.assert_array_equal(M.word_add(a, b, bits), M.element_add(a, b, bits))
    assert M.top_bits(bits) == {8: 0x8080808080808080, 16: 0x8000800080008000,
                                32: 0x8000000080000000, 64: 1 << 63}[bits]


@pytest.mark.parametrize("xor", [False, True])
@pytest.mark.parametrize("bits", [8, 16, 32, 64])
@pytest.mark.parametrize("nv", [4, 2])
def test_butterfly_gives_per_element_sums_in_the_lanes_the_kernel_reads(nv, bits, xor):
    """64 random lanes of NV words (4: a pair of leaf blocks; 2: the lone block
    of a tree without levels).  Word o's total over the 64 lanes, element by
    element mod 2^bits, ends in every lane with lane >> (6 - log2 NV) == o."""
    rng = np.random.default_rng(nv * 100 + bits)
    v = rng.integers(0, 1 << 64, size=(64, nv), dtype=np.uint64)
    v[5] = M.M64
    shift = 6 - int(np.log2(nv))
    for live in (64, 37):
        v[live:] = 0           # lanes past the last key hold zeros
        if xor:
            want = np.bitwise_xor.reduce(v, axis=0)
        else:
            elems = np.ascontiguousarray(v).view(M.DTYPE[bits]).reshape(64, -1)
            want = elems.sum(axis=0, dtype=M.DTYPE[bits]).view(np.uint64)
        got = M.butterfly(v, bits, xor)
        np.testing.assert_array_equal(got, want[np.arange(64) >> shift])
