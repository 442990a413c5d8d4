"""Checked private histograms (dpf_hip_expand_sketch,
EvaluateFullDomainSumSketch[ToDevice], histogram.fold_checked / check /
reconstruct_mod) as far as they can be checked without a GPU: the C ABI's
declarations, the supported types, the workspace size, the launch plan against
a Python restatement (with its threshold hook), the argument checks and their
order in both layers, and a NumPy model of the kernel's cross-lane reduction
that pins its lane map."""
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
SYMBOLS = ("dpf_hip_expand_sketch", "dpf_hip_expand_sketch_supported",
           "dpf_hip_expand_sketch_plan", "dpf_hip_expand_sketch_workspace_bytes")
WAVE_ITEMS_PER_CU = 64   # DPF_HIP_EXPAND_SKETCH_WAVE_ITEMS_PER_CU
MAX_LOG = 28             # DPF_HIP_EXPAND_SKETCH_MAX_LOG_DOMAIN
GROUP = 1                # levels of a leaf group: pairs
HOOK = "DPF_EXPAND_SKETCH_WAVE_ITEMS"
M32 = (1 << 32) - 5      # shift 0
M17 = 65537              # shift 15
MODN64 = 18446744073709551557


def _modn(*mods, blocks=2):
    return hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 32, m) for m in mods], False, 1, blocks)


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
    header = open(hip_abi.HEADER).read()
    assert "#define DPF_HIP_EXPAND_SKETCH_WAVE_ITEMS_PER_CU %d\n" % WAVE_ITEMS_PER_CU in header
    assert "#define DPF_HIP_EXPAND_SKETCH_MAX_LOG_DOMAIN %d\n" % MAX_LOG in header
    assert hip_abi.EXPAND_SKETCH_WAVE_ITEMS_PER_CU == WAVE_ITEMS_PER_CU
    assert hip_abi.EXPAND_SKETCH_MAX_LOG_DOMAIN == MAX_LOG
    for f in ("evaluate_full_domain_sum_sketch_to_device", "evaluate_full_domain_sum_sketch",
              "evaluates_full_domain_sum_sketch_on_device", "check_full_domain_sum_sketch_args"):
        assert hasattr(D.DistributedPointFunction, f), f
    for f in ("fold_checked", "check", "reconstruct_mod"):
        assert hasattr(HG, f), f


def test_supported_types():
    ok = hip_abi.expand_sketch_supported
    assert np.uint32(M32).item().bit_length() == 32 and M17.bit_length() == 17
    for d in (_modn(M32), _modn(M32, blocks=1), _modn(M17), _modn(M17, blocks=1),
              _modn(M32, M32), _modn(M17, M17), _modn(M32, M17), _modn(M17, M32)):
        assert ok(d)
    u64 = hip_abi.value_desc([(hip_abi.LEAF_INT, 64, 0)], True, 2, 1)
    xor = hip_abi.value_desc([(hip_abi.LEAF_XOR, 64, 0)], True, 2, 1)
    modn64 = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN64)], False, 1, 1)
    for d in (u64, xor, _modn(M32, M32, M32), modn64):
        assert not ok(d)
    assert not ok(None)
    # dpf_hip_expand_sum keeps refusing what this call takes.
    assert not hip_abi.expand_sum_supported(_modn(M32))
    assert not hip_abi.expand_sum_supported(_modn(M32, M32))


# ---- the workspace ---------------------------------------------------------------
def _workspace(K, n, nl, J):
    kp = -(-K // 64) * 64
    N = 1 << n
    return kp * (20 * n + 12) + 8 * N * nl + 8 * kp * J * nl + 4 * N * J * nl


def test_workspace_bytes_values_monotone_and_domain():
    w = hip_abi.expand_sketch_workspace_bytes
    keys = (0, 1, 63, 64, 65, 128, 129, 4096, 1 << 20, (1 << 31) - 1)
    for n in (1, 2, 7, 16, MAX_LOG):
        for nl in (1, 2):
            for J in (0, 1, 2):
                sizes = [w(k, n, n, nl, J) for k in keys]
                assert sizes == [_workspace(k, n, nl, J) for k in keys]
                assert sizes == sorted(sizes) and all(s % 8 == 0 for s in sizes)
                assert sizes[0] == (8 * nl + 4 * J * nl) << n     # no key: the accumulator only
    for k in keys:
        for nl in (1, 2):
            by_n = [w(k, n, n, nl, 2) for n in range(1, MAX_LOG + 1)]
            assert by_n == sorted(by_n)
            by_j = [w(k, 9, 9, nl, J) for J in (0, 1, 2)]
            assert by_j == sorted(by_j)
        assert w(k, 9, 9, 1, 2) < w(k, 9, 9, 2, 2)
    assert w(1, 1, 1, 1, 0) == 64 * 32 + 16
    for bad in ((-1, 4, 4, 1, 0), (1 << 31, 4, 4, 1, 0), (4, 0, 0, 1, 0), (4, 29, 29, 1, 0),
                (4, 3, 4, 1, 0), (4, 5, 4, 1, 0), (4, 4, 4, 0, 0), (4, 4, 4, 3, 0),
                (4, 4, 4, 1, -1), (4, 4, 4, 1, 3)):
        assert w(*bad) == -1, bad


# ---- the plan ---------------------------------------------------------------------
def _plan(num_keys, depth, num_cus, threshold=None):
    """dpf_hip_expand_sketch_plan restated."""
    chunks = -(-num_keys // 64)
    group = min(depth, GROUP)
    want = WAVE_ITEMS_PER_CU * num_cus if threshold is None else min(threshold, 1 << 24)
    walk = 0
    while walk < depth - group and (chunks << walk) < want:
        walk += 1
    return {"S": depth - walk, "walk": walk, "subtrees": 1 << walk, "wave_items": chunks << walk,
            "group": group, "threshold": want}


@pytest.mark.parametrize("num_cus", [256, 8])
@pytest.mark.parametrize("num_keys", [1, 63, 64, 65, 130, 4096, 1 << 20, (1 << 31) - 1])
def test_plan_equals_its_restatement(num_keys, num_cus, monkeypatch):
    monkeypatch.delenv(HOOK, raising=False)
    for depth in range(0, MAX_LOG + 1):
        pl = hip_abi.expand_sketch_plan(num_keys, depth, num_cus)
        assert pl == _plan(num_keys, depth, num_cus), depth
        assert pl["walk"] + pl["S"] == depth and pl["S"] >= pl["group"]
        assert pl["walk"] <= depth - pl["group"] if depth else pl["walk"] == 0


def test_plan_small_case_and_the_group_bound(monkeypatch):
    """tree_depth 0 has no level for a leaf pair: group = S = walk = 0 whatever
    the batch.  tree_depth 1 (n = 1) is exactly one pair: nothing is walked.
    Few keys of a deep tree stop at tree_depth - group, short of the threshold."""
    monkeypatch.delenv(HOOK, raising=False)
    for K in (1, 64, 65, 1 << 20):
        for cus in (8, 256):
            chunks = -(-K // 64)
            assert hip_abi.expand_sketch_plan(K, 0, cus) == {
                "S": 0, "walk": 0, "subtrees": 1, "wave_items": chunks, "group": 0,
                "threshold": WAVE_ITEMS_PER_CU * cus}
            pl = hip_abi.expand_sketch_plan(K, 1, cus)
            assert (pl["S"], pl["walk"], pl["group"], pl["wave_items"]) == (1, 0, 1, chunks)
    pl = hip_abi.expand_sketch_plan(1, 10, 256)
    assert (pl["walk"], pl["S"], pl["wave_items"]) == (9, 1, 512) and pl["wave_items"] < pl["threshold"]
    pl = hip_abi.expand_sketch_plan(64, 20, 256)
    assert (pl["walk"], pl["S"]) == (14, 6) and pl["wave_items"] == pl["threshold"] == 16384


def test_plan_threshold_hook(monkeypatch):
    """DPF_EXPAND_SKETCH_WAVE_ITEMS replaces the whole launch's threshold: 1
    walks nothing, 4 chunks' worth forces walk == 2 for any batch."""
    for K in (1, 63, 64, 65, 130):
        chunks = -(-K // 64)
        for t in (1, 4 * chunks, 5, 1 << 30):
            monkeypatch.setenv(HOOK, str(t))
            for depth in (0, 1, 2, 3, 6, 10):
                assert hip_abi.expand_sketch_plan(K, depth, 256) == _plan(K, depth, 256, t), (K, t)
        monkeypatch.setenv(HOOK, "1")
        assert hip_abi.expand_sketch_plan(K, 10, 256)["walk"] == 0
        monkeypatch.setenv(HOOK, str(4 * chunks))
        assert hip_abi.expand_sketch_plan(K, 10, 256)["walk"] == 2
        assert hip_abi.expand_sketch_plan(K, 2, 256)["walk"] == 1      # the group bound
    for unset in ("", "0", "-3"):
        monkeypatch.setenv(HOOK, unset)
        assert hip_abi.expand_sketch_plan(64, 10, 8) == _plan(64, 10, 8)


def test_plan_bad_shapes(monkeypatch):
    monkeypatch.delenv(HOOK, raising=False)
    for args in ((0, 8, 256), (-1, 8, 256), (1 << 31, 8, 256), (1, -1, 256), (1, MAX_LOG + 1, 256),
                 (1, 8, 0), (1, 8, -4), (1, 8, 65537)):
        with pytest.raises(hip_abi.DpfHipError) as e:
            hip_abi.expand_sketch_plan(*args)
        assert e.value.code == INVALID_ARGUMENT, args
    assert hip_abi.load().dpf_hip_expand_sketch_plan(1, 8, 256, None) == INVALID_ARGUMENT


# ---- dpf_hip_expand_sketch: every check before the device is touched -----------------
_RAW = (ctypes.c_uint64 * 66)()
_BASE = (ctypes.addressof(_RAW) + 15) & ~15     # a 16-byte aligned dummy, never read


def _abi_args(desc=None, null_desc=False, **over):
    """A call of dpf_hip_expand_sketch whose pointers are non-null, 16-byte
    aligned dummies: it must be rejected before anything dereferences them."""
    p = ctypes.c_void_p(_BASE)
    key = hip_abi.aes_key(0)
    kp = ctypes.cast(ctypes.pointer(key), ctypes.c_void_p)
    d = desc if desc is not None else _modn(M32, M32)
    a = dict(num_keys=2, num_levels=8, cw_stride=8, log_domain_size=8, key_seed=p, party=p,
             cw_seed=p, cw_left=p, cw_right=p, kl=kp, kr=kp, kv=kp,
             desc=ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), vcw=p, num_weights=2,
             weights=p, workspace=p,
             workspace_bytes=hip_abi.expand_sketch_workspace_bytes(2, 8, 8, 2, 2) - 1,
             sum_out=p, sketch_out=p, accumulate=1, stream=None)
    a.update(over)
    if null_desc:
        a["desc"] = None
    return list(a.values()), (key, d)


def _call(**over):
    """The default call is valid up to its workspace, one byte short: a call
    that passes every earlier check ends RESOURCE_EXHAUSTED, before the device."""
    lib = hip_abi.load()
    args, keep = _abi_args(**over)
    st = lib.dpf_hip_expand_sketch(*args)
    return st, lib.dpf_hip_last_error().decode()


def test_the_dummy_call_stops_at_the_workspace():
    need = hip_abi.expand_sketch_workspace_bytes(2, 8, 8, 2, 2)
    st, msg = _call()
    assert st == RESOURCE_EXHAUSTED and str(need) in msg
    for over in (dict(workspace_bytes=0), dict(workspace=None, workspace_bytes=need)):
        st, msg = _call(**over)
        assert st == RESOURCE_EXHAUSTED and str(need) in msg, over
    # J = 0 needs neither weights nor a sketch buffer, and a smaller workspace.
    need0 = hip_abi.expand_sketch_workspace_bytes(2, 8, 8, 2, 0)
    st, msg = _call(num_weights=0, weights=None, sketch_out=None, workspace_bytes=need0 - 1)
    assert st == RESOURCE_EXHAUSTED and str(need0) in msg
    st, msg = _call(desc=_modn(M17), workspace_bytes=0)
    assert st == RESOURCE_EXHAUSTED and str(hip_abi.expand_sketch_workspace_bytes(2, 8, 8, 1, 2)) in msg


@pytest.mark.parametrize("over", [
    # 1. sizes
    dict(num_keys=-1), dict(num_keys=1 << 31), dict(log_domain_size=0, num_levels=0),
    dict(log_domain_size=29, num_levels=29), dict(num_levels=7), dict(num_levels=9),
    # 2. desc and AES keys
    dict(kl=None), dict(kr=None), dict(kv=None), dict(null_desc=True),
    # 4. num_weights, 5. cw_stride, 6. outputs and weights
    dict(num_weights=-1), dict(num_weights=3), dict(cw_stride=7), dict(sum_out=None),
    dict(weights=None), dict(sketch_out=None), dict(num_weights=1, weights=None),
    # 8. key arrays
    dict(key_seed=None), dict(party=None), dict(cw_seed=None), dict(cw_left=None),
    dict(cw_right=None), dict(vcw=None),
], ids=str)
def test_argument_errors_are_invalid_argument(over):
    st, msg = _call(**over)
    assert st == INVALID_ARGUMENT and msg


def test_unsupported_types_are_unimplemented():
    u64 = hip_abi.value_desc([(hip_abi.LEAF_INT, 64, 0)], True, 2, 1)
    xor = hip_abi.value_desc([(hip_abi.LEAF_XOR, 64, 0)], True, 2, 1)
    modn64 = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 64, MODN64)], False, 1, 1)
    for d in (u64, xor, _modn(M32, M32, M32), modn64):
        st, msg = _call(desc=d)
        assert st == UNIMPLEMENTED and "IntModN<uint32_t, N>" in msg


def test_empty_batch_returns_ok_without_a_launch():
    """7. accumulate set: `sum_out` is left as it is, and nothing touches a device."""
    assert _call(num_keys=0)[0] == 0
    assert _call(num_keys=0, sketch_out=None)[0] == 0     # no key, no sketch to write
    assert _call(num_keys=0, key_seed=None, party=None, vcw=None, workspace=None,
                 workspace_bytes=0)[0] == 0


def test_misaligned_buffers_are_invalid_argument():
    """10. With a workspace large enough, alignment is what is left."""
    need = hip_abi.expand_sketch_workspace_bytes(2, 8, 8, 2, 2)
    for over in (dict(sum_out=ctypes.c_void_p(_BASE + 8)), dict(workspace=ctypes.c_void_p(_BASE + 8)),
                 dict(sum_out=ctypes.c_void_p(_BASE + 4)), dict(weights=ctypes.c_void_p(_BASE + 2)),
                 dict(sketch_out=ctypes.c_void_p(_BASE + 1))):
        st, msg = _call(workspace_bytes=need, **over)
        assert st == INVALID_ARGUMENT and "aligned" in msg, over


def test_two_faults_report_the_earlier_check():
    u64 = hip_abi.value_desc([(hip_abi.LEAF_INT, 64, 0)], True, 2, 1)
    by8 = ctypes.c_void_p(_BASE + 8)
    # 1 before 2, 3.
    assert "num_keys" in _call(num_keys=-1, kl=None, desc=u64)[1]
    assert "log_domain_size" in _call(log_domain_size=0, num_levels=0, desc=u64)[1]
    assert "num_levels" in _call(num_levels=7, null_desc=True)[1]
    # 2 before 3.
    assert _call(kl=None, desc=u64)[0] == INVALID_ARGUMENT
    # 3 before 4, 5, 6.
    for over in (dict(num_weights=3), dict(cw_stride=0), dict(sum_out=None)):
        assert _call(desc=u64, **over)[0] == UNIMPLEMENTED, over
    # 4 before 5, 5 before 6.
    assert "num_weights" in _call(num_weights=3, cw_stride=0)[1]
    assert "cw_stride" in _call(cw_stride=0, sum_out=None)[1]
    # 3 to 6 before 7: an empty batch still has them checked.
    assert _call(num_keys=0, desc=u64)[0] == UNIMPLEMENTED
    for over in (dict(num_weights=3), dict(cw_stride=7), dict(sum_out=None), dict(weights=None)):
        assert _call(num_keys=0, **over)[0] == INVALID_ARGUMENT, over
    # 7 before 8, 9, 10: an empty batch returns OK whatever the arrays.
    assert _call(num_keys=0, key_seed=None, workspace=None, sum_out=by8)[0] == 0
    # 8 before 9.
    st, msg = _call(party=None, workspace_bytes=0)
    assert st == INVALID_ARGUMENT and "NULL" in msg
    # 9 before 10.
    assert _call(workspace_bytes=0, sum_out=by8)[0] == RESOURCE_EXHAUSTED


# ---- the host API: every check before the device is touched, in order ---------------
LEVEL_MSG = "`hierarchy_level` must be non-negative and less than parameters_.size()"
TYPE_MSG = ("the checked full-domain sum is implemented for IntModN<uint32_t, N> and 2-tuples of "
            "it only")
DOMAIN_MSG = "the checked full-domain sum takes a log_domain_size in [1, 28]"
ROWS_MSG = "`num_weight_rows` must be in [0, 2]"
NULL_SUM_MSG = "`device_sum` must not be null"
NULL_W_MSG = "`device_weights` and `device_sketch` must not be null when num_weight_rows > 0"
SUM_MSG = "device sum buffer too small"
SKETCH_MSG = "device sketch buffer too small"
BATCH_MSG = "key batch does not match this DistributedPointFunction"
ALIGN_MSG = "`device_sum` must be aligned to 16 bytes, `device_weights` and `device_sketch` to 4"
HH_VT = ("tuple", [("intmodn", 32, M32)] * 2)


def _raised(call):
    with pytest.raises(D.DpfStatusError) as e:
        call()
    return e.value.code, e.value.message


def test_evaluates_on_device_by_type_and_level():
    for vt, n, want in ((("intmodn", 32, M32), 8, True), (("intmodn", 32, M17), 8, True),
                        (HH_VT, 8, True), (("tuple", [("intmodn", 32, M17)] * 2), 8, True),
                        (HH_VT, 1, True), (HH_VT, MAX_LOG, True), (HH_VT, MAX_LOG + 1, False),
                        (HH_VT, 0, False), (("int", 64), 8, False), (("xor", 64), 8, False),
                        (("intmodn", 64, MODN64), 8, False),
                        (("tuple", [("intmodn", 32, M32)] * 3), 8, False)):
        dpf = make([(n, vt, 0)])
        assert dpf.evaluates_full_domain_sum_sketch_on_device(0) is want, (vt, n)
        assert dpf.evaluates_full_domain_sum_sketch_on_device(1) is False
        assert dpf.evaluates_full_domain_sum_sketch_on_device(-1) is False
        # The two calls' types are disjoint.
        assert not (want and dpf.evaluates_full_domain_sum_on_device(0))
    two = make([(4, ("int", 64), 0), (10, HH_VT, 0)])
    assert [two.evaluates_full_domain_sum_sketch_on_device(h) for h in (0, 1)] == [False, True]


def test_host_checks_report_the_first_failing_one():
    """Level, value type and n <= 28, J, null pointers, the sum's size, the
    sketches' size, the batch, alignment: each tripped alone, and two faults at
    once report the earlier."""
    K, n, nl, J = 3, 8, 2, 2
    N = 1 << n
    dpf = make([(n, HH_VT, 0)])
    raw = torch.zeros(N * nl + 8, dtype=torch.int32)
    base = raw.data_ptr() + (-raw.data_ptr() % 16)       # 16-byte aligned, N * nl words follow
    w = (base, J * N * 4)
    s = (base, N * nl * 4)
    k = (base, K * J * nl * 4)

    def check(h=0, w=w, J=J, s=s, k=k, keys=K, matches=True, obj=dpf):
        return _raised(lambda: obj.check_full_domain_sum_sketch_args(keys, h, w, J, s, k,
                                                                     batch_matches=matches))

    dpf.check_full_domain_sum_sketch_args(K, 0, w, J, s, k)          # the valid call passes
    dpf.check_full_domain_sum_sketch_args(0, 0, w, J, s, (base, 0))  # and an empty batch
    dpf.check_full_domain_sum_sketch_args(0, 0, w, J, s, None)       # which has no sketch to write
    dpf.check_full_domain_sum_sketch_args(K, 0, None, 0, s, None)    # and the plain sum
    dpf.check_full_domain_sum_sketch_args(K, 0, w, 1, s, (base + 4, K * nl * 4))
    # Each check alone.
    assert check(h=1) == (INVALID_ARGUMENT, LEVEL_MSG)
    assert check(obj=make([(n, ("int", 64), 0)])) == (UNIMPLEMENTED, TYPE_MSG)
    assert check(obj=make([(MAX_LOG + 1, HH_VT, 0)]), s=(base, 1 << 40)) == \
        (INVALID_ARGUMENT, DOMAIN_MSG)
    for bad in (-1, 3):
        assert check(J=bad) == (INVALID_ARGUMENT, ROWS_MSG)
    assert check(s=(0, s[1])) == (INVALID_ARGUMENT, NULL_SUM_MSG)
    assert check(w=None) == (INVALID_ARGUMENT, NULL_W_MSG)
    assert check(k=(0, k[1])) == (INVALID_ARGUMENT, NULL_W_MSG)
    assert check(s=(base, s[1] - 1)) == (INVALID_ARGUMENT, SUM_MSG)
    assert check(k=(base, k[1] - 1)) == (INVALID_ARGUMENT, SKETCH_MSG)
    assert check(keys=-1) == (INVALID_ARGUMENT, SKETCH_MSG)
    assert check(matches=False) == (INVALID_ARGUMENT, BATCH_MSG)
    for over in (dict(s=(base + 8, s[1])), dict(w=(base + 2, w[1])), dict(k=(base + 1, k[1]))):
        assert check(**over) == (INVALID_ARGUMENT, ALIGN_MSG), over
    # The level, with every later fault present too.
    for h in (-1, 1):
        assert check(h=h, J=3, s=(0, 8), matches=False) == (INVALID_ARGUMENT, LEVEL_MSG)
    # The value type and its domain before J and the null pointer.
    for vt in (("int", 64), ("xor", 64), ("intmodn", 64, MODN64),
               ("tuple", [("intmodn", 32, M32)] * 3)):
        assert check(obj=make([(n, vt, 0)]), J=3, s=(0, 8), matches=False) == \
            (UNIMPLEMENTED, TYPE_MSG)
    assert check(obj=make([(MAX_LOG + 1, HH_VT, 0)]), J=3, s=(0, 8)) == \
        (INVALID_ARGUMENT, DOMAIN_MSG)
    # J before the null pointers, those before the sizes, the sum's before the sketches'.
    assert check(J=3, s=(0, 8)) == (INVALID_ARGUMENT, ROWS_MSG)
    assert check(s=(0, 8), w=None) == (INVALID_ARGUMENT, NULL_SUM_MSG)
    assert check(w=None, s=(base, 8)) == (INVALID_ARGUMENT, NULL_W_MSG)
    assert check(s=(base, 8), k=(base, 8), matches=False) == (INVALID_ARGUMENT, SUM_MSG)
    # The sketches' size before the batch, the batch before alignment.
    assert check(k=(base + 1, 8), matches=False) == (INVALID_ARGUMENT, SKETCH_MSG)
    assert check(s=(base + 8, s[1]), matches=False) == (INVALID_ARGUMENT, BATCH_MSG)
    # An empty batch still has its arguments checked.
    assert check(keys=0, s=(0, s[1])) == (INVALID_ARGUMENT, NULL_SUM_MSG)
    # Larger buffers than needed are fine.
    dpf.check_full_domain_sum_sketch_args(K, 0, w, J, (base, s[1] + 64), (base, k[1] + 64))


def test_full_domain_sum_still_refuses_the_field_types():
    for vt in (("intmodn", 32, M32), HH_VT):
        dpf = make([(8, vt, 0)])
        raw = torch.zeros(1 << 9, dtype=torch.int64)
        code, msg = _raised(lambda: dpf.check_full_domain_sum_args(3, 0, raw))
        assert code == UNIMPLEMENTED and "uint64_t and XorWrapper<uint64_t> only" in msg


# ---- histogram.reconstruct_mod -------------------------------------------------------------
def test_reconstruct_mod_on_hand_made_shares():
    a = np.array([[1, 2], [M32 - 1, M17 - 1], [M32 - 1, 0], [0, 0]], dtype=np.uint32)
    b = np.array([[2, 3], [1, 1], [M32 - 1, M17 - 1], [0, 0]], dtype=np.uint32)
    want = np.array([[3, 5], [0, 0], [M32 - 2, M17 - 1], [0, 0]], dtype=np.uint32)
    got = HG.reconstruct_mod(a, b, [M32, M17])
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, want)
    # int32 storage (torch has no uint32 arithmetic) and torch tensors are taken as their bits.
    np.testing.assert_array_equal(
        HG.reconstruct_mod(a.view(np.int32), torch.from_numpy(b.view(np.int32)), [M32, M17]), want)
    np.testing.assert_array_equal(HG.reconstruct_mod(a[:, 0], b[:, 0], [M32]), want[:, :1])


# ---- the cross-lane reduction ---------------------------------------------------------------
def _shfl_xor(x, off):
    """x[lane] -> x[lane ^ off] for an array whose first axis is the 64 lanes."""
    return x[np.arange(64) ^ off]


def _reduce_lanes(v):
    """reduce_lanes (dpf_expand_sketch.hip) on v[lane][value], NV = 2 nl values
    per lane (a leaf pair: leaf 0's nl elements, then leaf 1's): log2 NV
    halving steps at offsets 32, 16 in which a lane keeps the upper half of its
    remaining values where its lane bit is set (the lower half where it is
    clear), sends the other half to its partner and adds what it gets; then the
    last value is summed over the remaining offsets.  Returns (the value every
    lane ends with, the number of 64-bit sums per lane)."""
    lanes = np.arange(64)
    v = v.copy()
    nv = v.shape[1]
    off, sums = 32, 0
    while nv > 1:
        half = nv // 2
        up = ((lanes & off) != 0)[:, None]
        send = np.where(up, v[:, :half], v[:, half:nv])
        keep = np.where(up, v[:, half:nv], v[:, :half])
        v = keep + _shfl_xor(send, off)
        sums += half
        nv, off = half, off // 2
    r = v[:, 0]
    while off > 0:
        r = r + _shfl_xor(r, off)
        sums += 1
        off //= 2
    return r, sums


@pytest.mark.parametrize("nl,sums", [(2, 7), (1, 6)])
def test_reduction_leaves_each_value_in_the_lanes_the_kernel_reads(nl, sums):
    """64 lanes x 2 nl values, each below 2^32 (the largest: 2^32 - 1 in every
    lane, whose total 64 (2^32 - 1) < 2^38 shows nothing wraps).  The total of
    value o ends in every lane with lane >> OSHIFT == o, OSHIFT = 4 for nl = 2
    and 5 for nl = 1; the first such lane adds it to accumulator word
    pair * 2 nl + o, i.e. leaf 2 pair + o / nl, element o % nl."""
    nv = 2 * nl
    oshift = 4 if nl == 2 else 5
    rng = np.random.default_rng(nv)
    v = rng.integers(0, 1 << 32, size=(64, nv), dtype=np.uint64)
    v[:, 0] = (1 << 32) - 1
    want = np.array([sum(int(x) for x in v[:, o]) for o in range(nv)], dtype=np.uint64)
    assert int(want[0]) == 64 * ((1 << 32) - 1) < 1 << 38
    got, count = _reduce_lanes(v)
    assert count == sums
    np.testing.assert_array_equal(got, want[np.arange(64) >> oshift])
    issuing = [lane for lane in range(64) if lane & ((1 << oshift) - 1) == 0]
    assert [lane >> oshift for lane in issuing] == list(range(nv))
    # Lanes past the last key hold zeros and change no total.
    v[37:] = 0
    want = v.sum(axis=0, dtype=np.uint64)
    np.testing.assert_array_equal(_reduce_lanes(v)[0], want[np.arange(64) >> oshift])
