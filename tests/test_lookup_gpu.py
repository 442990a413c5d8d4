"""Batched private table lookup on an MI355X (dpf_hip_lookup_batch through
evaluate_lookup_batch_to_device and lookup.py): bit-exact against the oracle's
EvaluateUntil folded on the host on small domains, byte for byte against the
single-key full-domain evaluation (itself oracle-verified) on shapes that take
every path of the launch plan -- several keys per wave, one wave per key,
several waves per key, with and without a depth-first subtree -- with the wrap
of the rotation inside a subtree, on a subtree boundary and inside a leaf block;
the item loop, the hierarchy and keys generated on the device."""
import functools

import numpy as np
import pytest

import oracle as O
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import lookup as LK
from keygen_common import seed_ints
from test_host_api_cpu import leaves_value
from test_key_batch_cpu import make, seeds_array

pytestmark = pytest.mark.gpu

MASK64 = (1 << 64) - 1
WIDTHS = (1, 2, 4)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@functools.lru_cache(maxsize=None)
def _table(n, w):
    """2^n rows of w words: random, shared by every test of that shape."""
    rng = np.random.default_rng(1000 * n + w)
    return rng.integers(0, 1 << 64, size=(1 << n, w), dtype=np.uint64)


def _fold(y, table, s, xor):
    """sum_i y[i] * T[(i + s) mod N] mod 2^64 (XOR_i y[i] & T[...]) per word."""
    N = y.shape[0]
    rows = table[(np.arange(N, dtype=np.uint64) + np.uint64(s % N)) % np.uint64(N)]
    if xor:
        return np.bitwise_xor.reduce(y[:, None] & rows, axis=0)
    return (y[:, None] * rows).sum(axis=0, dtype=np.uint64)


def _run(dpf, dev, h, offsets, table, w, prefill=0xAB):
    """uint64 (K, w) through the device call, `out` prefilled."""
    import torch
    K = dev.num_keys
    out = torch.full((K * w * 8,), prefill, dtype=torch.uint8, device="cuda")
    assert dpf.evaluate_lookup_batch_to_device(dev, h, _dev(offsets), _dev(table), w, out) == K * w
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64).reshape(K, w)


def _beta(vt, k):
    return ((0x9E3779B97F4A7C15 * (k + 1)) & MASK64) | 1


@functools.lru_cache(maxsize=None)
def _oracle_case(n, vt):
    """Five keys of both parties at the edge alphas, and the oracle's full
    domain for each: computed once, shared by the table widths."""
    levels = [(n, vt, 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    N = 1 << n
    rng = np.random.default_rng(n * 7 + (vt[0] == "xor"))
    alphas = [0, 1 % N, N // 2, N - 1, int(rng.integers(0, N))]
    K = len(alphas)
    betas = [_beta(vt, k) for k in range(K)]
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
    offsets = np.array([0, 1, N - 1, N // 2, N + 3 + (5 << 40)], dtype=np.uint64)
    return dpf, host, alphas, betas, offsets, ys


@pytest.mark.parametrize("vt", [("int", 64), ("xor", 64)], ids=str)
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8])
def test_oracle_parity_both_parties(n, vt):
    dpf, host, alphas, betas, offsets, ys = _oracle_case(n, vt)
    assert dpf.evaluates_lookup_on_device(0)
    xor = vt[0] == "xor"
    N = 1 << n
    for w in WIDTHS:
        table = _table(n, w)
        shares = []
        for party in (0, 1):
            dev = dpf.upload_key_batch(host[party])
            got = _run(dpf, dev, 0, offsets, table, w)
            want = np.stack([_fold(ys[party][k], table, int(offsets[k]), xor)
                             for k in range(len(alphas))])
            np.testing.assert_array_equal(got, want, err_msg=f"party {party} W={w}")
            shares.append(got)
        total = LK.reconstruct(shares[0], shares[1], xor)
        for k, (a, b) in enumerate(zip(alphas, betas)):
            row = table[(a + int(offsets[k])) % N]
            want = (np.uint64(b) & row) if xor else (np.uint64(b) * row)
            np.testing.assert_array_equal(total[k], want, err_msg=f"key {k} W={w}")


# ---- every path of the plan -----------------------------------------------------
def _scan():
    cus = _cus()
    return {(n, K): hip_abi.lookup_plan(K, n - 1, 1, cus)
            for n in range(2, 18) for K in (1, 70, 300)}


def _class(pl):
    L = pl["items_per_key"]
    return "<64" if L < 64 else ("==64" if L == 64 else ">64")


def test_the_scan_meets_every_class_on_this_device():
    classes = {_class(pl) for pl in _scan().values()}
    assert classes == {"<64", "==64", ">64"}


def _shapes():
    """One shape of each class of the scan, K = 70 where the class has one (a
    partly filled last wave), the largest domain of the class: the deepest
    subtree.  Then the shape of the protocol, many keys of a small domain, in
    which the items visit subtrees depth-first with several keys per wave."""
    scan = _scan()
    picked = []
    for c in ("<64", "==64", ">64"):
        of = [(n, K) for (n, K), pl in scan.items() if _class(pl) == c]
        with70 = [s for s in of if s[1] == 70]
        picked.append(max(with70 or of))
    return picked + [(8, 1 << 14)]


def _sampled(K):
    return sorted({0, 1, 2, K // 3, K // 2, K - 3, K - 2, K - 1} & set(range(K)))[:8]


def _wrap_offsets(n, S, K, keys, rng):
    """Offsets of all keys; the sampled ones put the wrap (element N - s) on a
    subtree boundary, inside a subtree, between the two elements of a leaf
    block, nowhere, and take a value >= N."""
    N, sub = 1 << n, 1 << (S + 1)
    off = rng.integers(0, 1 << 63, size=K, dtype=np.uint64)
    special = [sub % N, (3 * sub + 2) % N, 1, N - 1, 0, (N // 2 + 1) % N, N + sub + 1 + (7 << 44),
               (N - sub) % N]
    for k, s in zip(keys, special):
        off[k] = s
    return off


def _single_key_reference(dpf, host, k, h, n):
    """Key k's full-domain evaluation through the single-key device path."""
    import torch
    key = dpf.key_from_batch(host, k)
    ctx = dpf.create_evaluation_context(key)
    out = torch.empty((1 << n) * 8, dtype=torch.uint8, device="cuda")
    assert dpf.evaluate_until_to_device(h, [], ctx, out) == 1 << n
    return out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("vt", [("int", 64), ("xor", 64)], ids=str)
@pytest.mark.parametrize("shape", range(4))
def test_every_path_against_the_single_key_evaluation(shape, vt):
    n, K = _shapes()[shape]
    xor = vt[0] == "xor"
    levels = [(n, vt, 0)]
    dpf = make(levels)
    rng = np.random.default_rng(n * 131 + K)
    alphas = np.zeros((K, 2), dtype=np.uint64)
    alphas[:, 0] = rng.integers(0, 1 << n, size=K, dtype=np.uint64)
    seeds = seeds_array(rng, K)
    host = dpf.generate_key_batch(alphas, [leaves_value(vt, [0x0123456789ABCDEF])],
                                  root_seeds=seeds)[shape % 2]
    dev = dpf.upload_key_batch(host)
    keys = _sampled(K)
    refs = {k: _single_key_reference(dpf, host, k, 0, n) for k in keys}
    for w in WIDTHS:
        pl = hip_abi.lookup_plan(K, n - 1, w, _cus())
        off = _wrap_offsets(n, pl["S"], K, keys, rng)
        got = _run(dpf, dev, 0, off, _table(n, w), w)
        for k in keys:
            want = _fold(refs[k], _table(n, w), int(off[k]), xor)
            assert got[k].tobytes() == want.tobytes(), (n, K, w, k, pl)


def test_the_shapes_take_every_path_on_this_device():
    """The classes of the scan, and both kinds of item -- one leaf block and a
    depth-first subtree -- below and above a wave per key."""
    cus = _cus()
    plans = [hip_abi.lookup_plan(K, n - 1, 1, cus) for n, K in _shapes()]
    assert [_class(pl) for pl in plans] == ["<64", "==64", ">64", "<64"]
    assert plans[2]["S"] > 0 and plans[3]["S"] > 0
    assert plans[0]["S"] == 0 or plans[1]["S"] == 0


# ---- the item loop ---------------------------------------------------------------
def test_dynamic_and_static_item_loops_agree(monkeypatch):
    """The smallest batch of 2^8-element keys whose launch gives every wave
    four chunks of 64 items: the same bytes with the loop dynamic (default)
    and with DPF_LOOKUP_DYNAMIC=0, each run reporting its own loop."""
    import torch
    cus, n, w = _cus(), 8, 1
    K = next(1 << e for e in range(8, 31)
             if hip_abi.lookup_plan(1 << e, n - 1, w, cus)["items"] >= cus * 4096)
    vt = ("int", 64)
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(5)
    alphas = np.zeros((K, 2), dtype=np.uint64)
    alphas[:, 0] = rng.integers(0, 1 << n, size=K, dtype=np.uint64)
    dev = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [3])],
                                           root_seeds=seeds_array(rng, K))[1]
    off = rng.integers(0, 1 << 63, size=K, dtype=np.uint64)
    outs = []
    for hook, dynamic in ((None, True), ("0", False)):
        if hook is None:
            monkeypatch.delenv("DPF_LOOKUP_DYNAMIC", raising=False)
        else:
            monkeypatch.setenv("DPF_LOOKUP_DYNAMIC", hook)
        outs.append(_run(dpf, dev, 0, off, _table(n, w), w))
        assert (hip_abi.last_dynamic_chunks() > 0) == dynamic, (K, hook)
    assert outs[0].tobytes() == outs[1].tobytes()
    # Against the single-key evaluation at the ends and in the middle.
    host = dpf.download_key_batch(dev)
    torch.cuda.synchronize()
    for k in (0, K // 2 + 1, K - 1):
        want = _fold(_single_key_reference(dpf, host, k, 0, n), _table(n, w), int(off[k]), False)
        assert outs[0][k].tobytes() == want.tobytes(), k


# ---- the hierarchy ---------------------------------------------------------------
@pytest.mark.parametrize("h", [0, 1])
def test_both_levels_of_an_incremental_dpf_match_the_oracle(h):
    vt = ("int", 64)
    levels = [(4, vt, 0), (10, vt, 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    n = levels[h][0]
    N = 1 << n
    rng = np.random.default_rng(40 + h)
    K = 6
    alphas = [int(a) for a in rng.integers(0, 1 << 10, size=K)]
    seeds = seeds_array(rng, K)
    betas = [[11], [13]]
    host = dpf.generate_key_batch(alphas, [leaves_value(vt, b) for b in betas], root_seeds=seeds)
    off = np.array([0, 1, N - 1, N + 2, 5, N // 2], dtype=np.uint64)
    shares = []
    for party in (0, 1):
        got = _run(dpf, dpf.upload_key_batch(host[party]), h, off, _table(n, 2), 2)
        for k in range(K):
            okey = O.generate_keys(P, alphas[k], betas, *seed_ints(seeds, k))[party]
            y = O.evaluate_until(P, h, [], O.create_context(P, okey))
            y = np.ascontiguousarray(y).view(np.uint64).reshape(N)
            np.testing.assert_array_equal(got[k], _fold(y, _table(n, 2), int(off[k]), False))
        shares.append(got)
    total = LK.reconstruct(shares[0], shares[1], False)
    for k in range(K):
        row = _table(n, 2)[((alphas[k] >> (10 - n)) + int(off[k])) % N]
        np.testing.assert_array_equal(total[k], np.uint64(betas[h][0]) * row)


# ---- the protocol, keys generated on the device ------------------------------------
@pytest.mark.parametrize("vt", [("int", 64), ("xor", 64)], ids=str)
def test_deal_evaluate_reconstruct_looks_up_the_table(vt):
    n, K, w = 8, 256, 2
    xor = vt[0] == "xor"
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(99)
    xs = [int(x) for x in rng.integers(0, 1 << n, size=K)]
    masks = [int(r) for r in rng.integers(0, 1 << n, size=K)]
    beta = MASK64 if xor else 1        # a lookup proper: the shares of T[x]
    d0, d1 = LK.deal(dpf, masks, [leaves_value(vt, [beta])])
    off = LK.offsets_for(xs, masks, n)
    table = _dev(_table(n, w))
    s0 = LK.evaluate(dpf, d0, off, table, w)
    s1 = LK.evaluate(dpf, d1, _dev(off), table, w)
    import torch
    torch.cuda.synchronize()
    np.testing.assert_array_equal(LK.reconstruct(s0, s1, xor), _table(n, w)[xs])


# ---- the host API on a real batch ---------------------------------------------------
def test_errors_of_the_real_call_and_the_host_returning_call():
    import torch
    n, K = 6, 3
    vt = ("int", 64)
    dpf, other = make([(n, vt, 0)]), make([(n + 1, vt, 0)])
    rng = np.random.default_rng(3)
    host = dpf.generate_key_batch([1, 2, 3], [leaves_value(vt, [9])], root_seeds=seeds_array(rng, K))
    dev = dpf.upload_key_batch(host[0])
    table, off = _dev(_table(n, 1)), _dev(np.arange(K, dtype=np.uint64))
    out = torch.zeros(K, dtype=torch.int64, device="cuda")

    def raised(call):
        with pytest.raises(D.DpfStatusError) as e:
            call()
        return e.value.code, e.value.message

    assert raised(lambda: dpf.evaluate_lookup_batch_to_device(dev, 0, off, table[:-1], 1, out)) == \
        (3, "`table_bytes` must be 2^log_domain_size * table_words * 8")
    assert raised(lambda: dpf.evaluate_lookup_batch_to_device(dev, 0, off, table, 1, out[:-1])) == \
        (3, "device output buffer too small")
    big = _dev(_table(n + 1, 1))
    assert raised(lambda: other.evaluate_lookup_batch_to_device(dev, 0, off, big, 1, out)) == \
        (3, "key batch does not match this DistributedPointFunction")
    assert raised(lambda: dpf.evaluate_lookup_batch(dev, 0, [1, 2], table, 1)) == \
        (3, "`offsets` must hold one offset per key of the batch")
    assert raised(lambda: dpf.evaluate_lookup_batch(dev, 0, [1, 2, 3], table, 3))[0] == 12
    # The host-returning call equals the device call.
    got = dpf.evaluate_lookup_batch(dev, 0, [0, 1, 2], table, 1)
    np.testing.assert_array_equal(got, _run(dpf, dev, 0, np.arange(K, dtype=np.uint64),
                                            _table(n, 1), 1))
    # An empty batch writes nothing and returns 0.
    empty = dpf.upload_key_batch(host[0], 0, 0)
    assert dpf.evaluate_lookup_batch_to_device(empty, 0, off, table, 1, out) == 0
    assert dpf.evaluate_lookup_batch(empty, 0, [], table, 1).shape == (0, 1)
