"""Fused full-domain sum over a key batch (dpf_hip_expand_sum,
EvaluateFullDomainSum[ToDevice], histogram.py) as far as it can be checked
without a GPU: the C ABI's declarations, the launch plan, the workspace size,
the argument checks and their order in both layers, histogram.reconstruct, and
a NumPy model of the kernel's halving butterfly that pins its lane map."""
import ctypes
import re

import numpy as np
import pytest
import torch

from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import histogram as HG
from test_key_batch_cpu import make

INVALID_ARGUMENT, RESOURCE_EXHAUSTED, UNIMPLEMENTED = 3, 8, 12
SYMBOLS = ("dpf_hip_expand_sum", "dpf_hip_expand_sum_supported", "dpf_hip_expand_sum_plan",
           "dpf_hip_expand_sum_workspace_bytes")
WAVE_ITEMS_PER_CU = 64   # DPF_HIP_EXPAND_SUM_WAVE_ITEMS_PER_CU
GROUP = 1                # levels of a leaf group: pairs
MODN = 18446744073709551557


def _desc(kind, bits):
    return hip_abi.value_desc([(kind, bits, 0)], True, 128 // bits, 1)


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
    assert hip_abi.EXPAND_SUM_WAVE_ITEMS_PER_CU == WAVE_ITEMS_PER_CU


def test_supported_types():
    for kind in (hip_abi.LEAF_INT, hip_abi.LEAF_XOR):
        assert hip_abi.expand_sum_supported(_desc(kind, 64))
        for bits in (8, 16, 32, 128):
            assert not hip_abi.expand_sum_supported(_desc(kind, bits)), (kind, bits)
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    pair64 = hip_abi.value_desc([(hip_abi.LEAF_INT, 64, 0)] * 2, True, 1, 1)
    for d in (modn, pair, pair64):
        assert not hip_abi.expand_sum_supported(d)
    assert not hip_abi.expand_sum_supported(None)


# ---- the plan ---------------------------------------------------------------------
@pytest.mark.parametrize("num_cus", [256, 8])
@pytest.mark.parametrize("num_keys", [1, 63, 64, 65, 4096, 1 << 20])
def test_plan_properties(num_keys, num_cus):
    chunks = -(-num_keys // 64)
    want = WAVE_ITEMS_PER_CU * num_cus
    for depth in range(0, 30):
        pl = hip_abi.expand_sum_plan(num_keys, depth, num_cus)
        S, walk, group = pl["S"], pl["walk"], pl["group"]
        assert walk + S == depth and S >= 0 and walk >= 0
        assert pl["subtrees"] == 2 ** walk
        assert pl["wave_items"] == chunks * 2 ** walk
        assert pl["threshold"] == want
        # The leaf group: pairs, or the whole of a tree that is shallower.
        assert group == min(depth, GROUP) and S >= group
        # The threshold rule: walk is the smallest value with enough wave items
        # for the dynamic loop, bounded by the levels the leaf group keeps.
        limit = depth - group
        if chunks * 2 ** limit < want:
            assert walk == limit, (depth, pl)
        else:
            assert pl["wave_items"] >= want, (depth, pl)
            assert walk == 0 or chunks * 2 ** (walk - 1) < want, (depth, pl)


def test_plan_small_cases():
    """D = 0 (n = 1): no tree, the root is value-hashed -- below the leaf
    group's depth, so the group is the whole tree and nothing is walked,
    whatever the batch; D = 1 is exactly one leaf group."""
    for K in (1, 64, 65, 1 << 20):
        for cus in (8, 256):
            chunks = -(-K // 64)
            assert hip_abi.expand_sum_plan(K, 0, cus) == {
                "S": 0, "walk": 0, "subtrees": 1, "wave_items": chunks, "group": 0,
                "threshold": WAVE_ITEMS_PER_CU * cus}
            pl = hip_abi.expand_sum_plan(K, GROUP, cus)
            assert (pl["S"], pl["walk"], pl["group"], pl["wave_items"]) == (GROUP, 0, GROUP, chunks)


def test_plan_bad_shapes():
    for args in ((0, 8, 256), (-1, 8, 256), (1 << 31, 8, 256), (1, -1, 256), (1, 30, 256),
                 (1, 8, 0), (1, 8, -4), (1, 8, 65537)):
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.expand_sum_plan(*args)
        assert e.value.code == INVALID_ARGUMENT, args
    assert hip_abi.load().dpf_hip_expand_sum_plan(1, 8, 256, None) == INVALID_ARGUMENT


def test_workspace_bytes_is_monotone():
    w = hip_abi.expand_sum_workspace_bytes
    keys = (0, 1, 63, 64, 65, 128, 129, 4096, 1 << 20, (1 << 31) - 1)
    for levels in range(0, 30):
        sizes = [w(k, levels) for k in keys]
        assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[1] > 0
        assert all(s % 16 == 0 for s in sizes)
    for k in keys:
        sizes = [w(k, levels) for levels in range(0, 30)]
        assert sizes == sorted(sizes)
    assert w(1, 0) == w(64, 0) == 64 * 20 and w(65, 3) == 128 * 20 * 4
    for bad in ((-1, 4), (1 << 31, 4), (4, -1), (4, 30)):
        assert w(*bad) == -1


# ---- dpf_hip_expand_sum: every check before the device is touched -------------------
_RAW = (ctypes.c_uint64 * 66)()
_BASE = (ctypes.addressof(_RAW) + 15) & ~15     # a 16-byte aligned dummy, never read


def _abi_args(desc=None, null_desc=False, **over):
    """A call of dpf_hip_expand_sum whose pointers are non-null, 16-byte aligned
    dummies: it must be rejected before anything dereferences them."""
    p = ctypes.c_void_p(_BASE)
    key = hip_abi.aes_key(0)
    kp = ctypes.cast(ctypes.pointer(key), ctypes.c_void_p)
    d = desc if desc is not None else _desc(hip_abi.LEAF_INT, 64)
    a = dict(num_keys=2, num_levels=7, cw_stride=7, log_domain_size=8, key_seed=p, party=p,
             cw_seed=p, cw_left=p, cw_right=p, kl=kp, kr=kp, kv=kp,
             desc=ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), vcw=p, workspace=p,
             workspace_bytes=hip_abi.expand_sum_workspace_bytes(2, 7), out=p, accumulate=1,
             stream=None)
    a.update(over)
    if null_desc:
        a["desc"] = None
    return list(a.values()), (key, d)


def _call(**over):
    lib = hip_abi.load()
    args, keep = _abi_args(**over)
    st = lib.dpf_hip_expand_sum(*args)
    return st, lib.dpf_hip_last_error().decode()


@pytest.mark.parametrize("over", [
    # 1. sizes
    dict(num_keys=-1), dict(num_keys=1 << 31), dict(log_domain_size=0, num_levels=-1),
    dict(log_domain_size=31, num_levels=30), dict(num_levels=8), dict(num_levels=6),
    # 2. desc and AES keys
    dict(kl=None), dict(kr=None), dict(kv=None), dict(null_desc=True),
    # 4. cw_stride, 5. out
    dict(cw_stride=6), dict(out=None),
    # 7. key arrays
    dict(key_seed=None), dict(party=None), dict(cw_seed=None), dict(cw_left=None),
    dict(cw_right=None), dict(vcw=None),
], ids=str)
def test_argument_errors_are_invalid_argument(over):
    st, msg = _call(**over)
    assert st == INVALID_ARGUMENT and msg


def test_unsupported_types_are_unimplemented():
    """3. uint32, uint128 and a tuple among them."""
    modn = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN)], False, 1, 1)
    pair = hip_abi.value_desc([(hip_abi.LEAF_INT, 32, 0)] * 2, True, 2, 1)
    for d in (_desc(hip_abi.LEAF_INT, 32), _desc(hip_abi.LEAF_INT, 128), pair, modn,
              _desc(hip_abi.LEAF_XOR, 128)):
        st, msg = _call(desc=d)
        assert st == UNIMPLEMENTED and "uint64_t" in msg


def test_empty_batch_returns_ok_without_a_launch():
    """6. accumulate set: `out` is left as it is, and nothing touches a device."""
    assert _call(num_keys=0)[0] == 0
    assert _call(num_keys=0, key_seed=None, party=None, vcw=None, workspace=None,
                 workspace_bytes=0)[0] == 0


def test_short_or_null_workspace_is_resource_exhausted():
    """8. The message names the size needed."""
    need = hip_abi.expand_sum_workspace_bytes(2, 7)
    for over in (dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace=None)):
        st, msg = _call(**over)
        assert st == RESOURCE_EXHAUSTED and str(need) in msg, over
    need = hip_abi.expand_sum_workspace_bytes(65, 7)
    st, msg = _call(num_keys=65)
    assert st == RESOURCE_EXHAUSTED and str(need) in msg


def test_misaligned_buffers_are_invalid_argument():
    """9."""
    for over in (dict(out=ctypes.c_void_p(_BASE + 8)), dict(workspace=ctypes.c_void_p(_BASE + 8)),
                 dict(out=ctypes.c_void_p(_BASE + 4))):
        st, msg = _call(**over)
        assert st == INVALID_ARGUMENT and "aligned" in msg, over


def test_no_tree_needs_no_correction_words():
    """n = 1: NULL correction words pass check 7; the call then stops at the
    short workspace, before the device."""
    st, _ = _call(log_domain_size=1, num_levels=0, cw_stride=0, cw_seed=None, cw_left=None,
                  cw_right=None, workspace_bytes=0)
    assert st == RESOURCE_EXHAUSTED
    assert _call(num_levels=7, cw_seed=None, workspace_bytes=0)[0] == INVALID_ARGUMENT


def test_two_faults_report_the_earlier_check():
    u32 = _desc(hip_abi.LEAF_INT, 32)
    by8 = ctypes.c_void_p(_BASE + 8)
    # 1 before 2, 3: a bad count with a NULL key and a bad type.
    assert _call(num_keys=-1, kl=None, desc=u32)[0] == INVALID_ARGUMENT
    assert "num_keys" in _call(num_keys=-1, desc=u32)[1]
    assert "log_domain_size" in _call(log_domain_size=0, num_levels=-1, desc=u32)[1]
    assert "num_levels" in _call(num_levels=6, null_desc=True)[1]
    # 2 before 3: a NULL AES key with an unsupported type.
    assert _call(kl=None, desc=u32)[0] == INVALID_ARGUMENT
    # 3 before 4 and 5: an unsupported type with a short stride, a NULL out.
    assert _call(desc=u32, cw_stride=0)[0] == UNIMPLEMENTED
    assert _call(desc=u32, out=None)[0] == UNIMPLEMENTED
    # 4 before 5: a short stride with a NULL out.
    assert "cw_stride" in _call(cw_stride=0, out=None)[1]
    # 3, 4, 5 before 6: an empty batch still has them checked.
    assert _call(num_keys=0, desc=u32)[0] == UNIMPLEMENTED
    assert _call(num_keys=0, cw_stride=6)[0] == INVALID_ARGUMENT
    assert _call(num_keys=0, out=None)[0] == INVALID_ARGUMENT
    # 6 before 7, 8, 9: an empty batch returns OK whatever the arrays.
    assert _call(num_keys=0, key_seed=None, workspace=None, out=by8)[0] == 0
    # 7 before 8: a NULL array with a short workspace.
    st, msg = _call(party=None, workspace_bytes=0)
    assert st == INVALID_ARGUMENT and "NULL" in msg
    # 8 before 9: a short workspace with a misaligned out.
    assert _call(workspace_bytes=0, out=by8)[0] == RESOURCE_EXHAUSTED


# ---- the host API: every check before the device is touched, in order ---------------
LEVEL_MSG = "`hierarchy_level` must be non-negative and less than parameters_.size()"
TYPE_MSG = "the full-domain sum is implemented for uint64_t and XorWrapper<uint64_t> only"
DOMAIN_MSG = "the full-domain sum takes a log_domain_size in [1, 30]"
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


def test_evaluates_full_domain_sum_on_device_by_type_and_level():
    for vt, n, want in ((("int", 64), 8, True), (("xor", 64), 8, True), (("int", 64), 1, True),
                        (("int", 64), 30, True), (("int", 64), 31, False), (("int", 64), 0, False),
                        (("int", 32), 8, False), (("int", 128), 8, False), (("xor", 128), 8, False),
                        (("intmodn", 64, MODN), 8, False),
                        (("tuple", [("int", 64), ("int", 64)]), 8, False)):
        dpf = make([(n, vt, 0)])
        assert dpf.evaluates_full_domain_sum_on_device(0) is want, (vt, n)
        assert dpf.evaluates_full_domain_sum_on_device(1) is False
        assert dpf.evaluates_full_domain_sum_on_device(-1) is False
    two = make([(4, ("int", 32), 0), (10, ("int", 64), 0)])
    assert [two.evaluates_full_domain_sum_on_device(h) for h in (0, 1)] == [False, True]


def test_host_checks_report_the_first_failing_one():
    """Level, value type (and its domain), null pointer, out_bytes, the batch,
    alignment: each tripped alone, and two faults at once report the earlier."""
    K, n = 3, 8
    N = 1 << n
    dpf = make([(n, ("int", 64), 0)])
    raw = torch.zeros(N + 4, dtype=torch.int64)
    shift = (-raw.data_ptr() % 16) // 8
    out = raw[shift:shift + N]                 # 16-byte aligned, N words
    assert out.data_ptr() % 16 == 0
    null = _Buffer(0, N * 8)
    misaligned = _Buffer(out.data_ptr() + 8, N * 8)

    def check(h=0, o=out, keys=K, matches=True, obj=dpf):
        return _raised(lambda: obj.check_full_domain_sum_args(keys, h, o, batch_matches=matches))

    dpf.check_full_domain_sum_args(K, 0, out)          # the valid call passes
    dpf.check_full_domain_sum_args(0, 0, out)          # and an empty batch
    # Each check alone.
    assert check(h=1) == (INVALID_ARGUMENT, LEVEL_MSG)
    assert check(obj=make([(n, ("int", 32), 0)])) == (UNIMPLEMENTED, TYPE_MSG)
    assert check(obj=make([(31, ("int", 64), 0)]), o=_Buffer(out.data_ptr(), 1 << 40)) == \
        (INVALID_ARGUMENT, DOMAIN_MSG)
    assert check(o=null) == (INVALID_ARGUMENT, NULL_MSG)
    assert check(o=out[:N - 1]) == (INVALID_ARGUMENT, OUT_MSG)
    assert check(keys=-1) == (INVALID_ARGUMENT, OUT_MSG)
    assert check(matches=False) == (INVALID_ARGUMENT, BATCH_MSG)
    assert check(o=misaligned) == (INVALID_ARGUMENT, ALIGN_MSG)
    # The level, with every later fault present too.
    for h in (-1, 1):
        assert check(h=h, o=_Buffer(0, 8), matches=False) == (INVALID_ARGUMENT, LEVEL_MSG)
    # The value type and its domain before the null pointer.
    for vt in (("int", 32), ("int", 128), ("xor", 128), ("intmodn", 64, MODN),
               ("tuple", [("int", 64), ("int", 64)])):
        assert check(obj=make([(n, vt, 0)]), o=_Buffer(0, 8), matches=False) == \
            (UNIMPLEMENTED, TYPE_MSG)
    assert check(obj=make([(0, ("int", 64), 0)]), o=null) == (INVALID_ARGUMENT, DOMAIN_MSG)
    assert check(obj=make([(31, ("int", 64), 0)]), o=null) == (INVALID_ARGUMENT, DOMAIN_MSG)
    # The null pointer before the output's size.
    assert check(o=_Buffer(0, 8), matches=False) == (INVALID_ARGUMENT, NULL_MSG)
    # The output's size before the batch.
    assert check(o=_Buffer(out.data_ptr() + 8, N * 8 - 8), matches=False) == \
        (INVALID_ARGUMENT, OUT_MSG)
    # The batch before alignment.
    assert check(o=misaligned, matches=False) == (INVALID_ARGUMENT, BATCH_MSG)
    # An empty batch still has its arguments checked.
    assert check(keys=0, o=null) == (INVALID_ARGUMENT, NULL_MSG)
    # A larger buffer than needed is fine.
    dpf.check_full_domain_sum_args(K, 0, _Buffer(out.data_ptr(), N * 8 + 64))


# ---- histogram.reconstruct ---------------------------------------------------------------
def test_reconstruct_on_hand_made_shares():
    top = (1 << 64) - 1
    a = np.array([1, top, 5, 1 << 63, 0], dtype=np.uint64)
    b = np.array([2, 1, top - 4, 1 << 63, 0], dtype=np.uint64)
    np.testing.assert_array_equal(HG.reconstruct(a, b, False),
                                  np.array([3, 0, 0, 0, 0], dtype=np.uint64))
    np.testing.assert_array_equal(HG.reconstruct(a, b, True),
                                  np.array([3, top - 1, 5 ^ (top - 4), 0, 0], dtype=np.uint64))
    # int64 storage (torch has no uint64 arithmetic) and torch tensors are taken as their bits.
    np.testing.assert_array_equal(HG.reconstruct(a.view(np.int64), torch.from_numpy(b.view(np.int64)),
                                                 False),
                                  np.array([3, 0, 0, 0, 0], dtype=np.uint64))
    assert HG.reconstruct(a, b, False).dtype == np.uint64


# ---- the halving butterfly ------------------------------------------------------------------
def _shfl_xor(x, off):
    """x[lane] -> x[lane ^ off] for an array whose first axis is the 64 lanes."""
    return x[np.arange(64) ^ off]


def _butterfly(v, xor):
    """reduce_lanes (dpf_expand_sum.hip) on v[lane][value], NV = 2^H values per
    lane: H halving steps at offsets 32, 16, ..., in which a lane keeps the
    upper half of its remaining values where its lane bit is set (the lower
    half where it is clear), sends the other half to its partner and adds what
    it gets; then the last value is summed over the remaining offsets.  Returns
    (the value every lane ends with, the number of 64-bit sums per lane)."""
    op = np.bitwise_xor if xor else np.add
    lanes = np.arange(64)
    v = v.copy()
    nv = v.shape[1]
    off, sums = 32, 0
    while nv > 1:
        half = nv // 2
        up = ((lanes & off) != 0)[:, None]
        send = np.where(up, v[:, :half], v[:, half:nv])
        keep = np.where(up, v[:, half:nv], v[:, :half])
        v = op(keep, _shfl_xor(send, off))
        sums += half
        nv, off = half, off // 2
    r = v[:, 0]
    while off > 0:
        r = op(r, _shfl_xor(r, off))
        sums += 1
        off //= 2
    return r, sums


@pytest.mark.parametrize("xor", [False, True])
@pytest.mark.parametrize("nv,sums", [(16, 17), (8, 10), (4, 7), (2, 6)])
def test_butterfly_leaves_each_output_in_the_lanes_the_kernel_reads(nv, sums, xor):
    """64 lanes x NV values (16: an octet's outputs, the widest group; 4: the
    pair the kernel uses; 2: the lone leaf block of n = 1).  The total of output
    o over the 64 lanes ends in every lane with lane >> (6 - log2 NV) == o, the
    first of which issues the atomic: lanes 4 o for 16 values, 16 o for 4."""
    rng = np.random.default_rng(nv)
    v = rng.integers(0, 1 << 64, size=(64, nv), dtype=np.uint64)
    want = np.bitwise_xor.reduce(v, axis=0) if xor else v.sum(axis=0, dtype=np.uint64)
    got, count = _butterfly(v, xor)
    assert count == sums
    shift = 6 - int(np.log2(nv))
    np.testing.assert_array_equal(got, want[np.arange(64) >> shift])
    issuing = [lane for lane in range(64) if lane & ((1 << shift) - 1) == 0]
    assert len(issuing) == nv and [lane >> shift for lane in issuing] == list(range(nv))
    # Lanes past the last key hold zeros and change no total.
    v[37:] = 0
    want = np.bitwise_xor.reduce(v, axis=0) if xor else v.sum(axis=0, dtype=np.uint64)
    np.testing.assert_array_equal(_butterfly(v, xor)[0], want[np.arange(64) >> shift])
