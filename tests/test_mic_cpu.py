"""MultipleIntervalContainmentGate (dcf/fss_gates/multiple_interval_containment
.{h,cc,proto}) on CPU: the reference's Create and Gen errors
(multiple_interval_containment_test.cc:210-481), the wire format of Interval /
MicParameters / MicKey, keys of the product Gen equal to the model's (mic_model,
over the oracle's DCF keygen) on the same seeds and mask shares, the offset
deduplication, the model's own reconstruction property, and the C ABI's
argument validation."""
import ctypes

import numpy as np
import pytest

import mic_model as MM
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import mic as M
from distributed_point_functions_amd import proto as pb

REF64 = [(10, 45), (23, 30), (45, 100), (66, 250), (15, 15)]   # test.cc:46-47
REF127 = [(2**126, 2**126 + 3), (2**127 - 1, 2**127 - 1), (2**127 - 3, 2**127 - 2)]  # :127-130


def gate(n, intervals):
    return M.MultipleIntervalContainmentGate.create(M.make_parameters(n, intervals))


def _interval(p, lower=None, upper=None):
    iv = p.intervals.add()
    if lower is not None:
        iv.lower_bound.value_uint128.low = lower
    if upper is not None:
        iv.upper_bound.value_uint128.low = upper
    return iv


@pytest.mark.parametrize("n,lower,upper,message", [
    (128, 10, 45, "log_group_size should be in > 0 and < 128"),        # test.cc:210-236
    (-1, 10, 45, "log_group_size should be in > 0 and < 128"),
    (20, 4, 1 << 20, "Interval bounds should be between 0 and 2\\^log_group_size"),  # :238-265
    (20, 1 << 20, 1 << 21, "Interval bounds should be between 0 and 2\\^log_group_size"),
    (20, 4, 3, "Interval upper bounds should be >= lower bound"),       # :267-293
    (20, None, 3, "Intervals should be non-empty"),                      # :295-318
    (20, 3, None, "Intervals should be non-empty"),
], ids=str)
def test_create_errors_match_reference(n, lower, upper, message):
    p = pb.MicParameters()
    p.log_group_size = n
    _interval(p, lower, upper)
    with pytest.raises(D.DpfStatusError, match=message) as e:
        M.MultipleIntervalContainmentGate.create(p)
    assert e.value.code == 3


def test_create_checks_run_in_reference_order():
    # cc:36-79: the group size before any interval, and per interval presence,
    # range, then order.
    p = pb.MicParameters()
    p.log_group_size = 128
    _interval(p, None, 3)
    with pytest.raises(D.DpfStatusError, match="log_group_size should be"):
        M.MultipleIntervalContainmentGate.create(p)
    p = pb.MicParameters()
    p.log_group_size = 4
    _interval(p, 20, 3)     # out of range and p > q: the range comes first
    with pytest.raises(D.DpfStatusError, match="Interval bounds should be between"):
        M.MultipleIntervalContainmentGate.create(p)
    p = pb.MicParameters()
    p.log_group_size = 4
    _interval(p, 5, 3)      # interval 0 fails its order check before interval 1's presence
    _interval(p, None, 3)
    with pytest.raises(D.DpfStatusError, match="Interval upper bounds should be >= lower bound"):
        M.MultipleIntervalContainmentGate.create(p)


def test_create_with_zero_group_size_fails_in_the_dcf():
    with pytest.raises(D.DpfStatusError, match="A DCF must have log_domain_size >= 1"):
        gate(0, [(0, 0)])


def test_gen_errors_match_reference():
    g = gate(64, REF64)
    with pytest.raises(D.DpfStatusError,
                       match="Count of output masks should be equal to the number of intervals"):
        g.gen(5, [1, 2, 3, 4])                                           # test.cc:320-374
    g = gate(10, [(10, 45)])
    with pytest.raises(D.DpfStatusError,
                       match="Input mask should be between 0 and 2\\^log_group_size"):
        g.gen(2048, [7])                                                 # :376-428
    with pytest.raises(D.DpfStatusError,
                       match="Output mask should be between 0 and 2\\^log_group_size"):
        g.gen(7, [2048])                                                 # :430-482
    # cc:106-126: the count is checked first, then r_in, then r_out.
    with pytest.raises(D.DpfStatusError, match="Count of output masks"):
        g.gen(2048, [2048, 1])
    with pytest.raises(D.DpfStatusError, match="Input mask should be"):
        g.gen(2048, [2048])


def test_messages_roundtrip_byte_equal_with_python_protobuf():
    host = D.host()
    p = M.make_parameters(127, REF127)
    one = p.intervals.add()
    one.upper_bound.value_uint128.low = 3        # only one bound set
    other = p.intervals.add()
    other.lower_bound.value_uint64 = 9           # the oneof's other member
    other.upper_bound.SetInParent()              # present and empty
    data = p.SerializeToString()
    assert bytes(host.roundtrip("MicParameters", data)) == data
    again = pb.MicParameters()
    again.ParseFromString(bytes(host.roundtrip("MicParameters", data)))
    assert again == p
    assert not again.intervals[3].HasField("lower_bound")
    assert again.intervals[3].HasField("upper_bound")
    for iv in p.intervals:
        d = iv.SerializeToString()
        assert bytes(host.roundtrip("Interval", d)) == d
    assert "upper_bound" in host.debug_string("Interval", one.SerializeToString())
    assert "lower_bound" not in host.debug_string("Interval", one.SerializeToString())

    g = gate(64, REF64)
    k0, k1 = g.gen(12345, [5, 6, 7, 8, 9], 3, 4, [2**63, 1, 0, 77, 2**64 - 1])
    for k in (k0, k1):
        d = k.SerializeToString()
        assert bytes(host.roundtrip("MicKey", d)) == d
        text = host.debug_string("MicKey", d)
        assert "dcfkey" in text and text.count("output_mask_share") == 5
    assert k0.dcfkey.key.party == 0 and k1.dcfkey.key.party == 1
    empty = pb.MicKey()
    assert bytes(host.roundtrip("MicKey", empty.SerializeToString())) == b""
    assert "log_group_size: 127" in host.debug_string("MicParameters", data)


@pytest.mark.parametrize("n,intervals", [(5, [(0, 0), (3, 9), (31, 31), (0, 31), (30, 31)]),
                                         (64, REF64), (127, REF127)], ids=["5", "64", "127"])
def test_gen_with_seeds_equals_model(n, intervals):
    rng = np.random.default_rng(n)
    N = 1 << n
    g = gate(n, intervals)
    m = len(intervals)
    for trial in range(4):
        big = lambda: int.from_bytes(rng.bytes(16), "little") % N   # noqa: E731
        r_in = [0, N - 1, big(), big()][trial]
        r_out = [big() for _ in range(m)]
        z_0 = [big() for _ in range(m)]
        s0, s1 = 100 + trial, 200 + trial
        keys = g.gen(r_in, r_out, s0, s1, z_0)
        model = MM.gen(n, intervals, r_in, r_out, s0, s1, z_0)
        for k, mk in zip(keys, model):
            dk = k.dcfkey.key
            assert D.u128_from_block(dk.seed) == mk["dcf"]["seed"]
            assert dk.party == mk["dcf"]["party"]
            cws = [(D.u128_from_block(c.seed), int(c.control_left), int(c.control_right))
                   for c in dk.correction_words]
            assert cws == [c[:3] for c in mk["dcf"]["cws"]]
            # Value corrections: level i < n - 1 in correction word i, the last level's apart.
            vcs = [[[D._get_integer(c.value_correction[0].integer)]] for c in dk.correction_words]
            assert vcs == [c[3] for c in mk["dcf"]["cws"]]
            assert [[D._get_integer(v.integer)] for v in dk.last_level_value_correction] == \
                mk["dcf"]["last_vc"]
            assert [D.u128_from_block(s.value_uint128) for s in k.output_mask_share] == mk["shares"]


def test_gen_without_seeds_is_random_and_consistent():
    n, intervals = 64, REF64
    g = gate(n, intervals)
    r_out = [1, 2, 3, 4, 5]
    a0, a1 = g.gen(99, r_out)
    b0, _ = g.gen(99, r_out)
    sh = lambda k: [D.u128_from_block(s.value_uint128) for s in k.output_mask_share]  # noqa: E731
    assert sh(a0) != sh(b0)                       # party 0's shares are fresh randomness
    assert a0.dcfkey.key.seed != b0.dcfkey.key.seed
    # z_0 + z_1 is the model's z whatever z_0 was.
    _, m1 = MM.gen(n, intervals, 99, r_out, 1, 2, [0] * 5)
    assert [(x + y) % 2**64 for x, y in zip(sh(a0), sh(a1))] == m1["shares"]
    assert all(s < 2**64 for s in sh(a0) + sh(a1))


def test_num_unique_offsets():
    for n in (3, 20, 127):
        N = 1 << n
        assert gate(n, [(0, N - 1)]).num_unique_offsets() == 1      # p = 0, q' = N mod N = 0
    for n, m in ((3, 8), (32, 8), (64, 64), (20, 5)):
        assert gate(n, MM.partition(n, m)).num_unique_offsets() == m
    rng = np.random.default_rng(1)
    for n, m in ((10, 5), (32, 8), (127, 3)):
        assert gate(n, MM.disjoint(n, m, rng)).num_unique_offsets() == 2 * m
    assert gate(5, [(0, 0), (3, 9), (31, 31), (0, 31), (30, 31)]).num_unique_offsets() == 6
    assert gate(7, []).num_unique_offsets() == 0


def test_make_key_batch_checks_share_count():
    g = gate(10, [(1, 2), (5, 9)])
    k0, k1 = g.gen(3, [4, 5], 1, 2, [6, 7])
    b = g.make_key_batch([k0, k1, k0])
    assert (b.num_keys, b.num_intervals) == (3, 2)
    assert MM.ints_of(b.mask_shares()) == [6, 7] + \
        [D.u128_from_block(s.value_uint128) for s in k1.output_mask_share] + [6, 7]
    assert b.dcf().num_keys == 3
    del k1.output_mask_share[1]
    with pytest.raises(D.DpfStatusError) as e:
        g.make_key_batch([k0, k1])
    assert e.value.code == 3


def test_model_reconstructs_exhaustively_at_n3():
    n, N = 3, 8
    rng = np.random.default_rng(3)
    intervals = [(p, q) for p in range(N) for q in range(p, N)]
    m = len(intervals)
    for r_in in (0, 5, 7):
        r_out = [int(v) for v in rng.integers(0, N, size=m)]
        z_0 = [int(v) for v in rng.integers(0, N, size=m)]
        k0, k1 = MM.gen(n, intervals, r_in, r_out, 11 + r_in, 22 + r_in, z_0)
        c0, c1 = {}, {}
        for x in range(N):
            xm = (x + r_in) % N
            got = MM.reconstruct(n, MM.evaluate(n, intervals, k0, xm, c0),
                                 MM.evaluate(n, intervals, k1, xm, c1), r_out)
            assert got == MM.contains(intervals, x), (r_in, x)


def _mic_abi_args(**over):
    """A call of dpf_hip_mic_eval_batch whose pointers are non-null dummies: it
    must be rejected before anything dereferences them."""
    blocks = (ctypes.c_uint64 * 64)()
    ptrs = (ctypes.c_void_p * 128)(*([ctypes.addressof(blocks)] * 128))
    p = ctypes.cast(blocks, ctypes.c_void_p)
    key = hip_abi.aes_key(0)
    a = dict(num_gates=4, n=8, key_seed=p, party=p, cw_seed=p, cw_left=p, cw_right=p, cw_stride=7,
             vcw=ctypes.cast(ptrs, ctypes.c_void_p), x=p, num_offsets=3, offsets=p,
             num_intervals=2, lower_index=p, upper_index=p, lower=p, upper_next=p, mask_share=p,
             scratch=p, kl=ctypes.cast(ctypes.pointer(key), ctypes.c_void_p),
             kr=ctypes.cast(ctypes.pointer(key), ctypes.c_void_p),
             kv=ctypes.cast(ctypes.pointer(key), ctypes.c_void_p), out=p, stream=None)
    a.update(over)
    return list(a.values()), (blocks, ptrs, key)


@pytest.mark.parametrize("over,message", [
    (dict(num_gates=-1), b"negative"),
    (dict(num_intervals=-1), b"negative"),
    (dict(n=0), b"log_group_size"),
    (dict(n=128), b"log_group_size"),
    (dict(cw_stride=6), b"cw_stride"),
    (dict(num_offsets=5), b"num_offsets"),
    (dict(num_offsets=0), b"num_offsets"),
    (dict(num_gates=2**60), b"too large"),
    (dict(x=None), b"NULL"),
    (dict(scratch=None), b"NULL"),
    (dict(lower_index=None), b"NULL"),
    (dict(mask_share=None), b"NULL"),
    (dict(out=None), b"NULL"),
    (dict(vcw=None), b"NULL"),
], ids=str)
def test_abi_validates_arguments_without_a_device(over, message):
    lib = hip_abi.load()
    args, keep = _mic_abi_args(**over)
    assert lib.dpf_hip_mic_eval_batch(*args) == 3
    assert message in lib.dpf_hip_last_error()


def test_abi_null_value_correction_level_and_empty_calls():
    lib = hip_abi.load()
    args, keep = _mic_abi_args()
    keep[1][5] = None                      # level 5's pointer
    assert lib.dpf_hip_mic_eval_batch(*args) == 3
    assert b"NULL value correction" in lib.dpf_hip_last_error()
    # Nothing to do: OK without touching a device, even with null arrays.
    for over in (dict(num_gates=0), dict(num_intervals=0, num_offsets=0)):
        args, keep = _mic_abi_args(x=None, out=None, scratch=None, **over)
        assert lib.dpf_hip_mic_eval_batch(*args) == 0
