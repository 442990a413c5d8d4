"""The packed full-domain sum on an MI355X (dpf_hip_expand_sum_packed through
evaluate_full_domain_sum_packed_to_device and histogram.py) for uint8/16/32/64
and XorWrapper of 8 to 128 bits: bit-exact against the oracle's EvaluateUntil
rows summed on the host, byte for byte against the batched prefix path's rows
on a shape of every class of the launch plan, carries that must stop at element
tops, many waves on one leaf group, `accumulate`, the 64-bit types against the
earlier call, the hierarchy, the item loop and histogram.fold.  Both group
operations are exact in any order: every comparison is an equality."""
import functools

import numpy as np
import pytest

import oracle as O
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import histogram as HG
from keygen_common import seed_ints
from test_host_api_cpu import leaves_value
from test_key_batch_cpu import make, seeds_array

pytestmark = pytest.mark.gpu

NINE = [("int", 8), ("int", 16), ("int", 32), ("int", 64),
        ("xor", 8), ("xor", 16), ("xor", 32), ("xor", 64), ("xor", 128)]
DTYPE = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64, 128: np.uint64}
GROUP = 1   # levels of the kernel's leaf group (pairs)


def _log2e(bits):
    return (128 // bits).bit_length() - 1


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _elements(raw, bits):
    """Packed bytes as elements: [N], or uint64 [N, 2] (low word first) for 128 bits."""
    a = np.ascontiguousarray(raw).reshape(-1).view(DTYPE[bits])
    return a.reshape(-1, 2) if bits == 128 else a


def _run(dpf, dev, h, n, bits, accumulate=False, prefill=0xAB, out=None):
    """The N packed elements through the device call; a fresh `out` is prefilled."""
    import torch
    if out is None:
        out = torch.full(((1 << n) * bits // 8,), prefill, dtype=torch.uint8, device="cuda")
    got = dpf.evaluate_full_domain_sum_packed_to_device(dev, h, out, accumulate=accumulate)
    assert got == 1 << n
    torch.cuda.synchronize()
    return _elements(out.cpu().numpy().copy(), bits)


def _group_sum(rows, bits, xor):
    """rows[key] of elements summed over the keys mod 2^bits, or XORed."""
    rows = np.asarray(rows, dtype=DTYPE[bits])
    return np.bitwise_xor.reduce(rows, axis=0) if xor else rows.sum(axis=0, dtype=DTYPE[bits])


def _packed(values, bits):
    """Python integers as packed elements."""
    raw = b"".join(int(v).to_bytes(bits // 8, "little") for v in values)
    return _elements(np.frombuffer(raw, dtype=np.uint8), bits)


def _histogram(n, alphas, betas, bits, xor):
    hist = [0] * (1 << n)
    for a, b in zip(alphas, betas):
        hist[a] = (hist[a] ^ b) if xor else ((hist[a] + b) & ((1 << bits) - 1))
    return _packed(hist, bits)


def _beta(k, bits):
    return ((0x9E3779B97F4A7C15F39CC0605CEDC835 * (k + 1)) & ((1 << bits) - 1)) | 1


def _batch_rows(dpf, dev, h, n, bits):
    """[key] rows of elements of a fresh batch context through the batched prefix path."""
    import torch
    K = dev.num_keys
    ctx = dpf.create_batch_evaluation_context(dev)
    out = torch.empty((K, (1 << n) * bits // 8), dtype=torch.uint8, device="cuda")
    assert dpf.evaluate_until_batch_to_device(h, [], ctx, out) == 1 << n
    torch.cuda.synchronize()
    rows = out.cpu().numpy().view(DTYPE[bits])
    return rows     # 128 bits: [K, 2 N] words, which XOR takes as they are


def _prefix_sum(dpf, dev, h, n, bits, xor):
    return _group_sum(_batch_rows(dpf, dev, h, n, bits), bits, xor).reshape(
        (-1, 2) if bits == 128 else (-1,))


# ---- 1. oracle parity ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(depth, vt):
    """Five keys of both parties at the edge alphas with odd betas, one of them
    all ones, and the oracle's full domain for each: computed once."""
    bits = vt[1]
    n = depth + _log2e(bits)
    levels = [(n, vt, 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    N = 1 << n
    rng = np.random.default_rng(depth * 7 + bits + (vt[0] == "xor"))
    alphas = [0, 1 % N, N // 2, N - 1, int(rng.integers(0, N))]
    K = len(alphas)
    betas = [_beta(k, bits) for k in range(K)]
    betas[1] = (1 << bits) - 1
    seeds = seeds_array(rng, K)
    values = [leaves_value(vt, [b]) for b in betas]
    host = dpf.generate_key_batch_with_betas(alphas, values, root_seeds=seeds)
    ys = []
    for party in (0, 1):
        rows = []
        for k in range(K):
            okey = O.generate_keys(P, alphas[k], [[betas[k]]], *seed_ints(seeds, k))[party]
            y = O.evaluate_until(P, 0, [], O.create_context(P, okey))
            rows.append(np.ascontiguousarray(y).reshape(-1).view(DTYPE[bits]).copy())
        ys.append(rows)
    return dpf, host, n, alphas, betas, ys


@pytest.mark.parametrize("vt", NINE, ids=str)
@pytest.mark.parametrize("depth", [0, 1, 2, 3, 6])
def test_oracle_parity_both_parties(depth, vt):
    """Tree depth n - log2 E: 0 is the root alone, 1 exactly one leaf group, 2
    and 3 a stack of one and two levels above the groups, 6 a deeper tree."""
    dpf, host, n, alphas, betas, ys = _oracle_case(depth, vt)
    bits, xor = vt[1], vt[0] == "xor"
    assert dpf.evaluates_full_domain_sum_packed_on_device(0)
    assert dpf.hierarchy_to_tree() == [depth]
    shares = []
    for party in (0, 1):
        got = _run(dpf, dpf.upload_key_batch(host[party]), 0, n, bits)
        want = _group_sum(ys[party], bits, xor).reshape(got.shape)
        np.testing.assert_array_equal(got, want, err_msg=f"party {party}")
        shares.append(got)
    np.testing.assert_array_equal(HG.reconstruct_packed(shares[0], shares[1], bits, xor),
                                  _histogram(n, alphas, betas, bits, xor))


# ---- 2. every class of the plan ---------------------------------------------------------
SCAN_KEYS = (1, 63, 64, 65, 130, 300)
PLAN_TYPES = [("int", 32), ("int", 8), ("xor", 16), ("xor", 128)]


def _dense_keys():
    """The smallest batch whose key chunks alone give the chip its wave items,
    so that nothing is walked (no batch of at most 300 keys does on a device
    of more than a few CUs)."""
    return 64 * hip_abi.EXPAND_SUM_WAVE_ITEMS_PER_CU * _cus()


def _scan():
    """The plan by tree depth, which is all it depends on: depths 1 to 13."""
    cus = _cus()
    keys = SCAN_KEYS + (_dense_keys(),)
    return {(d, K): hip_abi.expand_sum_plan(K, d, cus) for d in range(1, 14) for K in keys}


CLASSES = {
    "walk == 0, stack >= 2": lambda d, K, pl: pl["walk"] == 0 and pl["S"] - pl["group"] >= 2,
    "walk > 0": lambda d, K, pl: pl["walk"] > 0,
    "partly filled last chunk": lambda d, K, pl: K % 64 != 0,
    "more than one chunk": lambda d, K, pl: K > 64,
}
# Which members of a class its shape is taken from, so that the four shapes
# differ: the dense batch at depth 3 (its rows are summed on the host), a whole
# chunk, a lone partly filled chunk, and the scan's largest batch.
PICK = {
    "walk == 0, stack >= 2": lambda d, K: d <= 3,
    "walk > 0": lambda d, K: K == 64,
    "partly filled last chunk": lambda d, K: K == 63,
    "more than one chunk": lambda d, K: K == max(SCAN_KEYS),
}


def _shape_of(name):
    """The class's shape: the deepest tree among the members PICK allows."""
    return max((d, K) for (d, K), pl in _scan().items()
               if CLASSES[name](d, K, pl) and PICK[name](d, K))


def test_the_scan_meets_every_class_on_this_device():
    scan = _scan()
    for name, member in CLASSES.items():
        assert any(member(d, K, pl) for (d, K), pl in scan.items()), name
    shapes = [_shape_of(name) for name in CLASSES]
    assert len(set(shapes)) == len(CLASSES)
    assert all(d <= 13 for d, _ in shapes)


@pytest.mark.parametrize("vt", PLAN_TYPES, ids=str)
@pytest.mark.parametrize("name", list(CLASSES), ids=str)
def test_every_class_against_the_batched_prefix_path(name, vt):
    depth, K = _shape_of(name)
    assert CLASSES[name](depth, K, hip_abi.expand_sum_plan(K, depth, _cus()))
    bits, xor = vt[1], vt[0] == "xor"
    n = depth + _log2e(bits)
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(depth * 131 + K % 9973 + bits)
    alphas = np.zeros((K, 2), dtype=np.uint64)
    alphas[:, 0] = rng.integers(0, 1 << n, size=K, dtype=np.uint64)
    beta = 0x0123456789ABCDEF0123456789ABCDEF & ((1 << bits) - 1)
    dev = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [beta])],
                                           root_seeds=seeds_array(rng, K))[len(name) % 2]
    got = _run(dpf, dev, 0, n, bits)
    want = _prefix_sum(dpf, dev, 0, n, bits, xor)
    assert got.tobytes() == want.tobytes(), (n, K)


# ---- 3. carries stop at element tops -------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16, 32])
def test_carries_do_not_cross_elements(bits):
    """130 keys (two chunks and two lanes) on one bin with betas alternating
    2^B - 1 and 1: the bin's total wraps 65 times, its neighbours in the word
    reconstruct to 0, and each party's pseudo-random shares -- which overflow
    every element of every word many times over -- equal the prefix path's."""
    vt = ("int", bits)
    n, K = 9, 130
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(31 + bits)
    alpha = 21 * 16 + 5
    alphas = [alpha] * K
    betas = [(1 << bits) - 1 if k % 2 == 0 else 1 for k in range(K)]
    d0, d1 = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [b]) for b in betas],
                                              root_seeds=seeds_array(rng, K))
    shares = []
    for dev in (d0, d1):
        got = _run(dpf, dev, 0, n, bits)
        np.testing.assert_array_equal(got, _prefix_sum(dpf, dev, 0, n, bits, False))
        shares.append(got)
    total = HG.reconstruct_packed(shares[0], shares[1], bits, False)
    want = np.zeros(1 << n, dtype=DTYPE[bits])
    want[alpha] = sum(betas) & ((1 << bits) - 1)
    assert sum(betas) >> bits == 65 and int(want[alpha]) == 0
    np.testing.assert_array_equal(total, want)
    # A total that is not zero, so that a lost bin would show: one more key.
    alphas, betas = alphas + [alpha], betas + [3]
    d0, d1 = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [b]) for b in betas],
                                              root_seeds=seeds_array(rng, K + 1))
    total = HG.reconstruct_packed(_run(dpf, d0, 0, n, bits), _run(dpf, d1, 0, n, bits), bits, False)
    want[alpha] = 3
    np.testing.assert_array_equal(total, want)


# ---- 4. many waves on one leaf group -----------------------------------------------------
@pytest.mark.parametrize("vt", [("int", 8), ("int", 16), ("int", 32), ("xor", 8)], ids=str)
@pytest.mark.parametrize("depth", [1, 0])
def test_contention_on_one_leaf_group(depth, vt):
    """64 * 48 keys generated on the device over a tree of one leaf group (or
    the root alone): 48 waves add into the same 32 (16) bytes, the additive
    8- and 16-bit ones by compare-exchange."""
    bits, xor = vt[1], vt[0] == "xor"
    n, K = depth + _log2e(bits), 64 * 48
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(53 + bits + depth)
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=K)]
    betas = [_beta(k, bits) for k in range(K)]
    d0, d1 = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [b]) for b in betas],
                                              root_seeds=seeds_array(rng, K))
    shares = []
    for dev in (d0, d1):
        got = _run(dpf, dev, 0, n, bits)
        np.testing.assert_array_equal(got, _prefix_sum(dpf, dev, 0, n, bits, xor))
        shares.append(got)
    np.testing.assert_array_equal(HG.reconstruct_packed(shares[0], shares[1], bits, xor),
                                  _histogram(n, alphas, betas, bits, xor))


# ---- 5. accumulate and the empty batch -----------------------------------------------------
@pytest.mark.parametrize("vt", NINE, ids=str)
def test_accumulate_and_overwrite(vt):
    import torch
    bits, xor = vt[1], vt[0] == "xor"
    n, K = 8, 150
    N = 1 << n
    nbytes = N * bits // 8
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(23 + bits)
    alphas = [int(a) for a in rng.integers(0, N, size=K)]
    host = dpf.generate_key_batch(alphas, [leaves_value(vt, [5])], root_seeds=seeds_array(rng, K))[0]
    whole = dpf.upload_key_batch(host)
    # Overwriting reads nothing of what the buffer held.
    a = _run(dpf, whole, 0, n, bits, prefill=0xAB)
    b = _run(dpf, whole, 0, n, bits, prefill=0x00)
    assert a.tobytes() == b.tobytes()
    # Two half batches, the second accumulated, equal the whole batch.
    first, second = dpf.upload_key_batch(host, 0, 70), dpf.upload_key_batch(host, 70, K)
    out = torch.full((nbytes,), 0x5C, dtype=torch.uint8, device="cuda")
    _run(dpf, first, 0, n, bits, out=out)
    halves = _run(dpf, second, 0, n, bits, accumulate=True, out=out)
    assert halves.tobytes() == a.tobytes()
    # Accumulating into a buffer of 0xFF bytes adds (XORs) element by element.
    fill = _elements(np.full(nbytes, 0xFF, dtype=np.uint8), bits)
    got = _run(dpf, whole, 0, n, bits, accumulate=True, prefill=0xFF)
    np.testing.assert_array_equal(got, (fill ^ a) if xor else (fill + a))
    # The empty batch: N zeros, or the buffer as it was; no kernel is launched.
    empty = dpf.upload_key_batch(host, 0, 0)
    assert empty.num_keys == 0
    zeros = np.zeros_like(a)
    np.testing.assert_array_equal(_run(dpf, empty, 0, n, bits, prefill=0xAB), zeros)
    np.testing.assert_array_equal(_run(dpf, empty, 0, n, bits, accumulate=True, prefill=0xFF), fill)
    host_empty = dpf.evaluate_full_domain_sum_packed(empty, 0)
    assert host_empty.dtype == DTYPE[bits] and host_empty.shape == a.shape
    np.testing.assert_array_equal(host_empty, zeros)
    # The host-returning call equals the device call.
    host_whole = dpf.evaluate_full_domain_sum_packed(whole, 0)
    assert host_whole.dtype == DTYPE[bits] and host_whole.shape == a.shape
    np.testing.assert_array_equal(host_whole, a)


# ---- 6. the 64-bit types give the earlier call's bytes ----------------------------------------
@pytest.mark.parametrize("vt", [("int", 64), ("xor", 64)], ids=str)
@pytest.mark.parametrize("n,K", [(1, 5), (2, 64), (9, 130), (13, 65)])
def test_64_bits_through_the_packed_call_equal_the_earlier_call(n, K, vt):
    import torch
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(n * 5 + K)
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=K)]
    betas = [_beta(k, 64) for k in range(K)]
    dev = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [b]) for b in betas],
                                           root_seeds=seeds_array(rng, K))[n % 2]
    out = torch.full(((1 << n) * 8,), 0xAB, dtype=torch.uint8, device="cuda")
    assert dpf.evaluate_full_domain_sum_to_device(dev, 0, out) == 1 << n
    torch.cuda.synchronize()
    earlier = out.cpu().numpy().view(np.uint64)
    assert _run(dpf, dev, 0, n, 64).tobytes() == earlier.tobytes()


# ---- 7. the hierarchy, keys generated on the device -------------------------------------------
@pytest.mark.parametrize("h", [0, 1])
def test_both_levels_of_an_incremental_dpf_match_the_oracle(h):
    levels = [(6, ("int", 32), 0), (11, ("xor", 16), 0)]
    dpf = make(levels)
    assert dpf.generates_keys_on_device()
    P = O.OracleParams(levels)
    n, vt = levels[h][0], levels[h][1]
    bits, xor = vt[1], vt[0] == "xor"
    rng = np.random.default_rng(40 + h)
    K = 6
    alphas = [int(a) for a in rng.integers(0, 1 << 11, size=K)]
    seeds = seeds_array(rng, K)
    betas = [[0xFFFFFFF1], [0x8001]]
    devs = dpf.generate_key_batch_to_device(
        alphas, [leaves_value(levels[i][1], betas[i]) for i in (0, 1)], root_seeds=seeds)
    shares = []
    for party in (0, 1):
        got = _run(dpf, devs[party], h, n, bits)
        rows = []
        for k in range(K):
            okey = O.generate_keys(P, alphas[k], betas, *seed_ints(seeds, k))[party]
            y = O.evaluate_until(P, h, [], O.create_context(P, okey))
            rows.append(np.ascontiguousarray(y).reshape(-1).view(DTYPE[bits]))
        np.testing.assert_array_equal(got, _group_sum(rows, bits, xor), err_msg=f"party {party}")
        shares.append(got)
    want = _histogram(n, [a >> (11 - n) for a in alphas], [betas[h][0]] * K, bits, xor)
    np.testing.assert_array_equal(HG.reconstruct_packed(shares[0], shares[1], bits, xor), want)


# ---- 8. the item loop ---------------------------------------------------------------------
def test_dynamic_and_static_item_loops_agree(monkeypatch):
    """uint16_t, 65 keys (two chunks, the second one key) of the smallest
    domain whose launch reaches chunked_shape's rule -- 4 chunks for each of
    the 16 waves of one workgroup per CU: the same bytes with the loop dynamic
    (default) and with DPF_EXPAND_SUM_DYNAMIC=0, each run reporting its own."""
    cus, K, bits = _cus(), 65, 16
    vt = ("int", bits)
    depth = next(d for d in range(1, 30)
                 if hip_abi.expand_sum_plan(K, d, cus)["wave_items"] >= cus * 16 * 4)
    pl = hip_abi.expand_sum_plan(K, depth, cus)
    assert pl["walk"] > 0 and pl["wave_items"] < 2 * cus * 16 * 4 and depth <= 19
    assert hip_abi.expand_sum_plan(K, depth - 1, cus)["wave_items"] < cus * 16 * 4
    n = depth + _log2e(bits)
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(5)
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=K)]
    betas = [_beta(k, bits) for k in range(K)]
    d0, d1 = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [b]) for b in betas],
                                              root_seeds=seeds_array(rng, K))
    outs = []
    for hook, dynamic in ((None, True), ("0", False)):
        if hook is None:
            monkeypatch.delenv("DPF_EXPAND_SUM_DYNAMIC", raising=False)
        else:
            monkeypatch.setenv("DPF_EXPAND_SUM_DYNAMIC", hook)
        outs.append(_run(dpf, d0, 0, n, bits))
        assert (hip_abi.last_dynamic_chunks() > 0) == dynamic, (n, hook)
    assert outs[0].tobytes() == outs[1].tobytes()
    monkeypatch.delenv("DPF_EXPAND_SUM_DYNAMIC", raising=False)
    total = HG.reconstruct_packed(outs[0], _run(dpf, d1, 0, n, bits), bits, False)
    np.testing.assert_array_equal(total, _histogram(n, alphas, betas, bits, False))


# ---- 9. histogram.py ---------------------------------------------------------------------------
@pytest.mark.parametrize("vt", [("int", 32), ("xor", 8)], ids=str)
def test_submit_fold_reconstruct_packed_round_trip(vt):
    import torch
    bits, xor = vt[1], vt[0] == "xor"
    n, K = 10, 200
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(99)
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=K)]
    beta = 1                      # a histogram proper: the count of every bin
    d0, d1 = HG.submit(dpf, alphas, [leaves_value(vt, [beta])])
    s0 = HG.fold(dpf, d0)
    # The second server streams its clients in as two batches of one accumulator.
    host1 = dpf.download_key_batch(d1)
    s1 = HG.fold(dpf, dpf.upload_key_batch(host1, 0, 64), accumulate=True)
    HG.fold(dpf, dpf.upload_key_batch(host1, 64, K), out=s1, accumulate=True)
    torch.cuda.synchronize()
    assert s0.shape == (1 << n,) and s0.dtype == {32: torch.int32, 8: torch.uint8}[bits]
    assert s1.shape == s0.shape and s1.dtype == s0.dtype
    got = HG.reconstruct_packed(s0, s1, bits, xor)
    assert got.dtype == DTYPE[bits]
    np.testing.assert_array_equal(got, _histogram(n, alphas, [beta] * K, bits, xor))


def test_fold_shapes_for_16_and_128_bits():
    import torch
    for vt, dtype, shape in ((("int", 16), torch.int16, (64,)), (("xor", 128), torch.int64, (64, 2))):
        dpf = make([(6, vt, 0)])
        d0, d1 = HG.submit(dpf, [3, 3, 60], [leaves_value(vt, [7])])
        s0, s1 = HG.fold(dpf, d0), HG.fold(dpf, d1)
        torch.cuda.synchronize()
        assert s0.dtype == dtype and tuple(s0.shape) == shape
        got = HG.reconstruct_packed(s0, s1, vt[1], vt[0] == "xor")
        np.testing.assert_array_equal(got, _histogram(6, [3, 3, 60], [7] * 3, vt[1], vt[0] == "xor"))
