"""Fused full-domain sum over a key batch on an MI355X (dpf_hip_expand_sum
through evaluate_full_domain_sum_to_device and histogram.py): bit-exact against
the oracle's EvaluateUntil rows summed on the host on small domains, byte for
byte against the batched prefix path (itself oracle-verified) on a shape of
every class of the launch plan, colliding alphas, `accumulate`, the empty
batch, the item loop, the hierarchy and keys generated on the device.  Both
group operations are exact in any order: every comparison is an equality."""
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

MASK64 = (1 << 64) - 1
TYPES = [("int", 64), ("xor", 64)]
GROUP = 1   # levels of the kernel's leaf group (pairs): 4 outputs


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(dpf, dev, h, n, accumulate=False, prefill=0xAB, out=None):
    """uint64 [2^n] through the device call; a fresh `out` is prefilled."""
    import torch
    if out is None:
        out = torch.full(((1 << n) * 8,), prefill, dtype=torch.uint8, device="cuda")
    assert dpf.evaluate_full_domain_sum_to_device(dev, h, out, accumulate=accumulate) == 1 << n
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64).copy()


def _group_sum(rows, xor):
    rows = np.asarray(rows, dtype=np.uint64)
    return np.bitwise_xor.reduce(rows, axis=0) if xor else rows.sum(axis=0, dtype=np.uint64)


def _histogram(n, alphas, betas, xor):
    hist = np.zeros(1 << n, dtype=np.uint64)
    for a, b in zip(alphas, betas):
        hist[a] = (int(hist[a]) ^ b) if xor else ((int(hist[a]) + b) & MASK64)
    return hist


def _beta(k):
    return ((0x9E3779B97F4A7C15 * (k + 1)) & MASK64) | 1


def _batch_rows(dpf, dev, h, n):
    """[key][element] of a fresh batch context through the batched prefix path."""
    import torch
    K = dev.num_keys
    ctx = dpf.create_batch_evaluation_context(dev)
    out = torch.empty((K, 1 << n), dtype=torch.int64, device="cuda")
    assert dpf.evaluate_until_batch_to_device(h, [], ctx, out) == 1 << n
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


# ---- 1. oracle parity ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(n, vt):
    """Five keys of both parties at the edge alphas with odd betas, and the
    oracle's full domain for each: computed once."""
    levels = [(n, vt, 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    N = 1 << n
    rng = np.random.default_rng(n * 7 + (vt[0] == "xor"))
    alphas = [0, 1 % N, N // 2, N - 1, int(rng.integers(0, N))]
    K = len(alphas)
    betas = [_beta(k) for k in range(K)]
    seeds = seeds_array(rng, K)
    values = [leaves_value(vt, [b]) for b in betas]
    host = dpf.generate_key_batch_with_betas(alphas, values, root_seeds=seeds)
    ys = []
    for party in (0, 1):
        rows = []
        for k in range(K):
            okey = O.generate_keys(P, alphas[k], [[betas[k]]], *seed_ints(seeds, k))[party]
            y = O.evaluate_until(P, 0, [], O.create_context(P, okey))
            rows.append(np.ascontiguousarray(y).view(np.uint64).reshape(N).copy())
        ys.append(rows)
    return dpf, host, alphas, betas, ys


@pytest.mark.parametrize("vt", TYPES, ids=str)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 10])
def test_oracle_parity_both_parties(n, vt):
    """n = 1 is the no-tree case, n = 2 exactly one leaf group, the others have
    a depth-first stack above the groups."""
    dpf, host, alphas, betas, ys = _oracle_case(n, vt)
    assert dpf.evaluates_full_domain_sum_on_device(0)
    xor = vt[0] == "xor"
    shares = []
    for party in (0, 1):
        got = _run(dpf, dpf.upload_key_batch(host[party]), 0, n)
        np.testing.assert_array_equal(got, _group_sum(ys[party], xor), err_msg=f"party {party}")
        shares.append(got)
    np.testing.assert_array_equal(HG.reconstruct(shares[0], shares[1], xor),
                                  _histogram(n, alphas, betas, xor))


# ---- 2. every class of the plan ---------------------------------------------------------
SCAN_KEYS = (1, 63, 64, 65, 130, 300)


def _dense_keys():
    """The smallest batch whose key chunks alone give the chip its wave items,
    so that nothing is walked.  With at most 300 keys the scan has at most 5
    chunks, which no device of more than a few CUs is filled by: on an MI355X
    the scan alone holds no launch with walk == 0 below a one-group tree, and
    this batch is added to it."""
    return 64 * hip_abi.EXPAND_SUM_WAVE_ITEMS_PER_CU * _cus()


def _scan():
    cus = _cus()
    keys = SCAN_KEYS + (_dense_keys(),)
    return {(n, K): hip_abi.expand_sum_plan(K, n - 1, cus) for n in range(2, 17) for K in keys}


CLASSES = {
    "walk == 0, stack >= 2": lambda n, K, pl: pl["walk"] == 0 and pl["S"] - pl["group"] >= 2,
    "walk > 0": lambda n, K, pl: pl["walk"] > 0,
    "partly filled last chunk": lambda n, K, pl: K % 64 != 0,
    "more than one chunk": lambda n, K, pl: K > 64,
}
# Which members of a class its shape is taken from, so that the four shapes
# differ: the dense batch at n <= 4 (its rows are summed on the host), a whole
# chunk, a lone partly filled chunk, and the scan's largest batch.
PICK = {
    "walk == 0, stack >= 2": lambda n, K: n <= 4,
    "walk > 0": lambda n, K: K == 64,
    "partly filled last chunk": lambda n, K: K == 63,
    "more than one chunk": lambda n, K: K == max(SCAN_KEYS),
}


def _shape_of(name):
    """The class's shape: the largest n <= 14 among the members PICK allows."""
    return max((n, K) for (n, K), pl in _scan().items()
               if CLASSES[name](n, K, pl) and PICK[name](n, K) and n <= 14)


def test_the_scan_meets_every_class_on_this_device():
    scan = _scan()
    for name, member in CLASSES.items():
        assert any(member(n, K, pl) for (n, K), pl in scan.items()), name
    # The scan proper (K <= 300) holds every class that a batch of at most 5
    # chunks can be in on this device, and a stack two deep below a walk.
    proper = {s: pl for s, pl in scan.items() if s[1] in SCAN_KEYS}
    for name in ("walk > 0", "partly filled last chunk", "more than one chunk"):
        assert any(CLASSES[name](n, K, pl) for (n, K), pl in proper.items()), name
    assert any(pl["walk"] > 0 and pl["S"] - pl["group"] >= 2 for pl in proper.values())
    # The four shapes differ, and each is in its class.
    shapes = [_shape_of(name) for name in CLASSES]
    assert len(set(shapes)) == len(CLASSES)


@pytest.mark.parametrize("vt", TYPES, ids=str)
@pytest.mark.parametrize("name", list(CLASSES), ids=str)
def test_every_class_against_the_batched_prefix_path(name, vt):
    n, K = _shape_of(name)
    assert CLASSES[name](n, K, hip_abi.expand_sum_plan(K, n - 1, _cus()))
    xor = vt[0] == "xor"
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(n * 131 + K % 9973)
    alphas = np.zeros((K, 2), dtype=np.uint64)
    alphas[:, 0] = rng.integers(0, 1 << n, size=K, dtype=np.uint64)
    dev = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [0x0123456789ABCDEF])],
                                           root_seeds=seeds_array(rng, K))[len(name) % 2]
    got = _run(dpf, dev, 0, n)
    want = _group_sum(_batch_rows(dpf, dev, 0, n), xor)
    assert got.tobytes() == want.tobytes(), (n, K)


# ---- 3. collisions ------------------------------------------------------------------------
@pytest.mark.parametrize("vt", TYPES, ids=str)
@pytest.mark.parametrize("spread", [1, 2 << GROUP, 16],
                         ids=["one alpha", "one leaf group", "16 outputs"])
def test_colliding_alphas(spread, vt):
    """130 keys (two chunks and two lanes) whose alphas are one bin, or lie
    inside the 4 outputs of one leaf group, or inside 16 consecutive outputs
    (four groups, one 128-byte line of the output)."""
    n, K = 9, 130
    xor = vt[0] == "xor"
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(17 + spread)
    base = 21 * 16
    alphas = [base + int(a) for a in rng.integers(0, spread, size=K)]
    betas = [_beta(k) for k in range(K)]
    d0, d1 = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [b]) for b in betas],
                                              root_seeds=seeds_array(rng, K))
    total = HG.reconstruct(_run(dpf, d0, 0, n), _run(dpf, d1, 0, n), xor)
    want = _histogram(n, alphas, betas, xor)
    np.testing.assert_array_equal(total, want)
    assert np.count_nonzero(want) <= spread
    if spread == 1:
        assert int(total[base]) == (int(np.bitwise_xor.reduce(np.array(betas, dtype=np.uint64)))
                                    if xor else sum(betas) & MASK64)


# ---- 4. accumulate and the empty batch -----------------------------------------------------
@pytest.mark.parametrize("vt", TYPES, ids=str)
def test_accumulate_and_overwrite(vt):
    import torch
    n, K = 8, 150
    N = 1 << n
    xor = vt[0] == "xor"
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(23)
    alphas = [int(a) for a in rng.integers(0, N, size=K)]
    host = dpf.generate_key_batch(alphas, [leaves_value(vt, [5])], root_seeds=seeds_array(rng, K))[0]
    whole = dpf.upload_key_batch(host)
    # Overwriting reads nothing of what the buffer held.
    a = _run(dpf, whole, 0, n, prefill=0xAB)
    b = _run(dpf, whole, 0, n, prefill=0x00)
    assert a.tobytes() == b.tobytes()
    # Two half batches, the second accumulated, equal the whole batch.
    first, second = dpf.upload_key_batch(host, 0, 70), dpf.upload_key_batch(host, 70, K)
    out = torch.full((N * 8,), 0x5C, dtype=torch.uint8, device="cuda")
    _run(dpf, first, 0, n, out=out)
    halves = _run(dpf, second, 0, n, accumulate=True, out=out)
    assert halves.tobytes() == a.tobytes()
    # Accumulating into a prefilled buffer adds (XORs) to what it holds.
    fill = np.full(N, 0xABABABABABABABAB, dtype=np.uint64)
    got = _run(dpf, whole, 0, n, accumulate=True, prefill=0xAB)
    np.testing.assert_array_equal(got, (fill ^ a) if xor else (fill + a))
    # The empty batch: N zeros, or the buffer as it was; no kernel is launched.
    empty = dpf.upload_key_batch(host, 0, 0)
    assert empty.num_keys == 0
    np.testing.assert_array_equal(_run(dpf, empty, 0, n, prefill=0xAB), np.zeros(N, dtype=np.uint64))
    np.testing.assert_array_equal(_run(dpf, empty, 0, n, accumulate=True, prefill=0xAB), fill)
    np.testing.assert_array_equal(dpf.evaluate_full_domain_sum(empty, 0), np.zeros(N, dtype=np.uint64))
    # The host-returning call equals the device call.
    np.testing.assert_array_equal(dpf.evaluate_full_domain_sum(whole, 0), a)


# ---- 5. the item loop ---------------------------------------------------------------------
def test_dynamic_and_static_item_loops_agree(monkeypatch):
    """65 keys (two chunks, the second one key) of the smallest domain whose
    launch reaches chunked_shape's rule -- 4 chunks for each of the 16 waves of
    one workgroup per CU, here wave items -- which is where the plan stops
    walking: the same bytes with the loop dynamic (default) and with
    DPF_EXPAND_SUM_DYNAMIC=0, each run reporting its own loop."""
    cus, K = _cus(), 65
    n = next(n for n in range(2, 30)
             if hip_abi.expand_sum_plan(K, n - 1, cus)["wave_items"] >= cus * 16 * 4)
    pl = hip_abi.expand_sum_plan(K, n - 1, cus)
    assert pl["walk"] > 0 and pl["wave_items"] < 2 * cus * 16 * 4 and n <= 20
    assert hip_abi.expand_sum_plan(K, n - 2, cus)["wave_items"] < cus * 16 * 4
    vt = ("int", 64)
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(5)
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=K)]
    betas = [_beta(k) for k in range(K)]
    d0, d1 = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [b]) for b in betas],
                                              root_seeds=seeds_array(rng, K))
    outs = []
    for hook, dynamic in ((None, True), ("0", False)):
        if hook is None:
            monkeypatch.delenv("DPF_EXPAND_SUM_DYNAMIC", raising=False)
        else:
            monkeypatch.setenv("DPF_EXPAND_SUM_DYNAMIC", hook)
        outs.append(_run(dpf, d0, 0, n))
        assert (hip_abi.last_dynamic_chunks() > 0) == dynamic, (n, hook)
    assert outs[0].tobytes() == outs[1].tobytes()
    monkeypatch.delenv("DPF_EXPAND_SUM_DYNAMIC", raising=False)
    total = HG.reconstruct(outs[0], _run(dpf, d1, 0, n), False)
    np.testing.assert_array_equal(total, _histogram(n, alphas, betas, False))


# ---- 6. the hierarchy, keys generated on the device -------------------------------------------
@pytest.mark.parametrize("h", [0, 1])
def test_both_levels_of_an_incremental_dpf_match_the_oracle(h):
    levels = [(6, ("int", 64), 0), (11, ("xor", 64), 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    n, vt = levels[h][0], levels[h][1]
    xor = vt[0] == "xor"
    N = 1 << n
    rng = np.random.default_rng(40 + h)
    K = 6
    alphas = [int(a) for a in rng.integers(0, 1 << 11, size=K)]
    seeds = seeds_array(rng, K)
    betas = [[11], [13]]
    host = dpf.generate_key_batch(alphas, [leaves_value(levels[i][1], betas[i]) for i in (0, 1)],
                                  root_seeds=seeds)
    shares = []
    for party in (0, 1):
        got = _run(dpf, dpf.upload_key_batch(host[party]), h, n)
        rows = []
        for k in range(K):
            okey = O.generate_keys(P, alphas[k], betas, *seed_ints(seeds, k))[party]
            y = O.evaluate_until(P, h, [], O.create_context(P, okey))
            rows.append(np.ascontiguousarray(y).view(np.uint64).reshape(N))
        np.testing.assert_array_equal(got, _group_sum(rows, xor), err_msg=f"party {party}")
        shares.append(got)
    want = _histogram(n, [a >> (11 - n) for a in alphas], [betas[h][0]] * K, xor)
    np.testing.assert_array_equal(HG.reconstruct(shares[0], shares[1], xor), want)


@pytest.mark.parametrize("vt", TYPES, ids=str)
def test_device_generated_keys_sum_and_reconstruct(vt):
    n, K = 7, 100
    xor = vt[0] == "xor"
    dpf = make([(n, vt, 0)])
    assert dpf.generates_keys_on_device()
    rng = np.random.default_rng(77)
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=K)]
    betas = [_beta(k) for k in range(K)]
    d0, d1 = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [b]) for b in betas])
    total = HG.reconstruct(_run(dpf, d0, 0, n), _run(dpf, d1, 0, n), xor)
    np.testing.assert_array_equal(total, _histogram(n, alphas, betas, xor))


# ---- 7. histogram.py ---------------------------------------------------------------------------
@pytest.mark.parametrize("vt", TYPES, ids=str)
def test_submit_fold_reconstruct_round_trip(vt):
    import torch
    n, K = 10, 200
    xor = vt[0] == "xor"
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
    assert s0.shape == (1 << n,) and s0.dtype == torch.int64
    np.testing.assert_array_equal(HG.reconstruct(s0, s1, xor), _histogram(n, alphas, [beta] * K, xor))
