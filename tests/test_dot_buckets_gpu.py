"""Multi-query PIR over a bucketed database on an MI355X: dpf_hip_expand_rows
bit-exact against the oracle and byte for byte against the single-key
evaluation on shapes that take every path of its plan; dpf_hip_dot_buckets
against the NumPy model of the segmented fold; evaluate_dot_buckets_to_device
key by key against evaluate_dot on the bucket's slice, chunked, queued back to
back and at the second level of a hierarchy; pir.py's batch-code protocol end
to end; and the calls that share the scratch, unchanged afterwards.  Every
output and workspace the tests own is poisoned before a call."""
import functools

import numpy as np
import pytest

import oracle as O
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import pir
from dot_buckets_model import bucket_of_keys, dot_buckets, expected_shape
from keygen_common import seed_ints
from test_host_api_cpu import leaves_value
from test_key_batch_cpu import make, seeds_array

pytestmark = pytest.mark.gpu

MASK64 = (1 << 64) - 1
KEYS = (O.PRG_KEY_LEFT, O.PRG_KEY_RIGHT, O.PRG_KEY_VALUE)
TYPES = [("int", 64), ("xor", 64)]
POISON = 0xAB


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _dev_u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _desc(vt):
    return hip_abi.value_desc(O.leaves(vt), True, 2, 1)


def _beta(k):
    return ((0x9E3779B97F4A7C15 * (k + 1)) & MASK64) | 1


def _combine(a, b, xor):
    return a ^ b if xor else a + b


# ---- expand_rows -------------------------------------------------------------------
def _expand_rows(host, n, vt, stride=None, cw_stride=None):
    """uint64 (K, N) through the C ABI from a host key batch's arrays, the
    rows (and the gap a larger stride leaves) poisoned first."""
    import torch
    K, N = host.num_keys, 1 << n
    stride = 8 * N if stride is None else stride
    rows = torch.full((K, stride // 8), -0x5454545454545455, dtype=torch.int64, device="cuda")
    L = host.num_levels if cw_stride is None else cw_stride
    empty = np.zeros(16, np.uint8)
    got = hip_abi.expand_rows(
        n, _dev(host.seeds()), _dev_u8(host.party()),
        _dev(host.cw_seeds()) if L else _dev(empty), _dev_u8(host.cw_left() if L else empty),
        _dev_u8(host.cw_right() if L else empty), KEYS, _desc(vt),
        _dev(host.value_correction(0)), rows=rows, row_stride_bytes=stride, cw_stride=L)
    torch.cuda.synchronize()
    full = got.cpu().numpy().view(np.uint64).reshape(K, stride // 8)
    assert (full[:, N:] == np.uint64(0xABABABABABABABAB)).all(), "bytes past 8 N were written"
    return full[:, :N]


@functools.lru_cache(maxsize=None)
def _oracle_case(n, vt):
    """Five keys of both parties at the edge alphas, and the oracle's full
    domain for each: computed once."""
    levels = [(n, vt, 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    N = 1 << n
    rng = np.random.default_rng(n * 7 + (vt[0] == "xor"))
    alphas = [0, 1 % N, N // 2, N - 1, int(rng.integers(0, N))]
    K = len(alphas)
    betas = [_beta(k) for k in range(K)]
    seeds = seeds_array(rng, K)
    host = dpf.generate_key_batch_with_betas(alphas, [leaves_value(vt, [b]) for b in betas],
                                             root_seeds=seeds)
    ys = []
    for party in (0, 1):
        rows = []
        for k in range(K):
            okey = O.generate_keys(P, alphas[k], [[betas[k]]], *seed_ints(seeds, k))[party]
            y = O.evaluate_until(P, 0, [], O.create_context(P, okey))
            rows.append(np.ascontiguousarray(y).view(np.uint64).reshape(N).copy())
        ys.append(np.stack(rows))
    return dpf, host, alphas, betas, ys


@pytest.mark.parametrize("vt", TYPES, ids=str)
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8])
def test_expand_rows_oracle_parity_both_parties(n, vt):
    dpf, host, alphas, betas, ys = _oracle_case(n, vt)
    xor = vt[0] == "xor"
    shares = []
    for party in (0, 1):
        got = _expand_rows(host[party], n, vt)
        np.testing.assert_array_equal(got, ys[party], err_msg=f"party {party}")
        shares.append(got)
    total = _combine(shares[0], shares[1], xor)
    want = np.zeros_like(total)
    for k, (a, b) in enumerate(zip(alphas, betas)):
        want[k, a] = b
    np.testing.assert_array_equal(total, want)


def _class(pl):
    L = pl["items_per_key"]
    return "<64" if L < 64 else ("==64" if L == 64 else ">64")


@functools.lru_cache(maxsize=None)
def _shapes():
    """The cheapest (K, n) of a scan for each class of the plan -- several
    keys per wave, one wave per key, several waves per key -- with one leaf
    block per item (S == 0) and with a depth-first subtree (S > 0), on this
    device.  The K of the scan are no multiples of 64 except 64 itself."""
    cus = _cus()
    best = {}
    for n in range(2, 15):
        for K in (1, 3, 64, 70, 300, 1030, 2100, 4200, 8400):
            pl = hip_abi.expand_rows_plan(K, n - 1, cus)
            c = (_class(pl), pl["S"] > 0)
            if c not in best or K << n < best[c][0] << best[c][1]:
                best[c] = (K, n)
    return best


def test_the_scan_meets_every_class_on_this_device():
    assert set(_shapes()) == {(c, s) for c in ("<64", "==64", ">64") for s in (False, True)}


def _single_key_reference(dpf, host, k, h, n):
    """Key k's full-domain evaluation through the single-key device path."""
    import torch
    key = dpf.key_from_batch(host, k)
    ctx = dpf.create_evaluation_context(key)
    out = torch.empty((1 << n) * 8, dtype=torch.uint8, device="cuda")
    assert dpf.evaluate_until_to_device(h, [], ctx, out) == 1 << n
    return out.cpu().numpy().view(np.uint64)


def _sampled(K):
    return sorted({0, 1, 2, 63, 64, 65, K // 3, K // 2, K - 3, K - 2, K - 1} & set(range(K)))


@pytest.mark.parametrize("vt", TYPES, ids=str)
@pytest.mark.parametrize("deep", [False, True], ids=["S0", "S>0"])
@pytest.mark.parametrize("cls", ["<64", "==64", ">64"])
def test_expand_rows_every_path_against_the_single_key_evaluation(cls, deep, vt):
    """Sampled keys byte for byte against EvaluateUntil, all rows at once
    against the fused full-domain sum of the batch; a row stride larger than
    8 N whose gap stays untouched."""
    K, n = _shapes()[(cls, deep)]
    xor = vt[0] == "xor"
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(n * 131 + K)
    alphas = np.zeros((K, 2), dtype=np.uint64)
    alphas[:, 0] = rng.integers(0, 1 << n, size=K, dtype=np.uint64)
    party = int(deep)
    host = dpf.generate_key_batch(alphas, [leaves_value(vt, [0x0123456789ABCDEF])],
                                  root_seeds=seeds_array(rng, K))[party]
    got = _expand_rows(host, n, vt, stride=8 * (1 << n) + 48)
    for k in _sampled(K):
        want = _single_key_reference(dpf, host, k, 0, n)
        assert got[k].tobytes() == want.tobytes(), (K, n, k)
    total = dpf.evaluate_full_domain_sum(dpf.upload_key_batch(host), 0)
    mine = np.bitwise_xor.reduce(got, axis=0) if xor else got.sum(axis=0, dtype=np.uint64)
    np.testing.assert_array_equal(mine, total)


def test_expand_rows_dynamic_and_static_item_loops_agree(monkeypatch):
    """A batch generated on the device, large enough for the dynamic loop:
    the same bytes with DPF_EXPAND_ROWS_DYNAMIC=0, each run reporting its own
    loop, and equal to the single-key evaluation."""
    import torch
    cus, n, vt = _cus(), 8, ("int", 64)
    K = next(1 << e for e in range(8, 31)
             if hip_abi.expand_rows_plan(1 << e, n - 1, cus)["items"] >= cus * 4096)
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(5)
    alphas = np.zeros((K, 2), dtype=np.uint64)
    alphas[:, 0] = rng.integers(0, 1 << n, size=K, dtype=np.uint64)
    dev = dpf.generate_key_batch_to_device(alphas, [leaves_value(vt, [3])],
                                           root_seeds=seeds_array(rng, K))[1]
    host = dpf.download_key_batch(dev)
    torch.cuda.synchronize()
    outs = []
    for hook, dynamic in ((None, True), ("0", False)):
        if hook is None:
            monkeypatch.delenv("DPF_EXPAND_ROWS_DYNAMIC", raising=False)
        else:
            monkeypatch.setenv("DPF_EXPAND_ROWS_DYNAMIC", hook)
        outs.append(_expand_rows(host, n, vt))
        assert (hip_abi.last_dynamic_chunks() > 0) == dynamic, (K, hook)
    assert outs[0].tobytes() == outs[1].tobytes()
    for k in (0, K // 2 + 1, K - 1):
        assert outs[0][k].tobytes() == _single_key_reference(dpf, host, k, 0, n).tobytes(), k


# ---- dot_buckets alone -------------------------------------------------------------
POPULATIONS = [0, 1, 17, 0, 65, 1]     # empty buckets, a tile boundary at 16, several passes
BEGIN = [0] + list(np.cumsum(POPULATIONS))
WIDTHS = (1, 2, 3, 4, 33, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def _fold_inputs(N, stride_words):
    rng = np.random.default_rng(N)
    K, B = BEGIN[-1], len(POPULATIONS)
    y = rng.integers(0, 1 << 64, size=(K, stride_words), dtype=np.uint64)
    db = rng.integers(0, 1 << 64, size=(B, N, max(WIDTHS)), dtype=np.uint64)
    return y, db


def _dot_buckets(n, W, begin, vt, y, db):
    """uint64 (K, W) through the C ABI, `out` and the workspace poisoned."""
    import torch
    K, B = begin[-1], len(begin) - 1
    need = hip_abi.dot_buckets_workspace_bytes(_desc(vt), W, B, K, n)
    assert need > 0
    ws = torch.full((need,), POISON, dtype=torch.uint8, device="cuda")
    out = torch.full((K, W), -0x5454545454545455, dtype=torch.int64, device="cuda")
    hip_abi.dot_buckets(n, W, begin, _desc(vt), _dev(y), y.shape[1] * 8, _dev(db), out=out,
                        workspace=ws)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("vt", TYPES, ids=str)
@pytest.mark.parametrize("n,stride_words", [(1, 2), (6, 64), (10, 1024 + 6), (13, 1 << 13)])
def test_dot_buckets_against_the_model(n, stride_words, vt):
    """Every width on the populations; at n = 10 (1000 rows rounded up to the
    domain, a stride larger than the row) and n = 13 a bucket's rows span
    several workgroups and meet by atomics, below they are stored."""
    N, xor = 1 << n, vt[0] == "xor"
    y, db_all = _fold_inputs(N, stride_words)
    if n == 10:
        y = y.copy()
        y[:, 1000:N] = 0       # 1000 records: the shares past them are zero
    for W in WIDTHS:
        db = np.ascontiguousarray(db_all[:, :, :W])
        got = _dot_buckets(n, W, BEGIN, vt, y, db)
        want = dot_buckets(y[:, :N], BEGIN, db, xor)
        np.testing.assert_array_equal(got, want, err_msg=f"W={W}")
        items, tiles, largest, chunks = hip_abi.last_dot_buckets_shape()
        assert (tiles, largest, chunks) == expected_shape(BEGIN, W)
        assert tiles == 1 + 2 + 5 + 1 and items % tiles == 0
        assert (items > tiles) == (n >= 10), (n, W, items)


@pytest.mark.parametrize("vt", TYPES, ids=str)
def test_dot_buckets_all_ones_carries(vt):
    n, W = 10, 3
    N = 1 << n
    y = np.full((BEGIN[-1], N), MASK64, dtype=np.uint64)
    db = np.full((len(POPULATIONS), N, W), MASK64, dtype=np.uint64)
    got = _dot_buckets(n, W, BEGIN, vt, y, db)
    np.testing.assert_array_equal(got, dot_buckets(y, BEGIN, db, vt[0] == "xor"))
    # (2^64 - 1)^2 = 1 mod 2^64, N times: N; the XOR of an even count of ones: 0.
    assert (got == (0 if vt[0] == "xor" else N)).all()


def test_dot_buckets_one_key_per_bucket_and_one_bucket():
    """The protocol's shape (a tile of one key per bucket) and its opposite
    (every key in the last bucket of three)."""
    n, W, vt = 8, 5, ("int", 64)
    rng = np.random.default_rng(8)
    for begin in (list(range(25)), [0, 0, 0, 40]):
        K, B = begin[-1], len(begin) - 1
        y = rng.integers(0, 1 << 64, size=(K, 1 << n), dtype=np.uint64)
        db = rng.integers(0, 1 << 64, size=(B, 1 << n, W), dtype=np.uint64)
        np.testing.assert_array_equal(_dot_buckets(n, W, begin, vt, y, db),
                                      dot_buckets(y, begin, db, False))
        assert hip_abi.last_dot_buckets_shape()[1:] == expected_shape(begin, W)


# ---- evaluate_dot_buckets_to_device ---------------------------------------------------
def _dirty_scratch(dpf, dev, h=0):
    """Leaves another call's table in the object's workspace."""
    if dev.num_keys:
        dpf.evaluate_full_domain_sum(dev, h)


def _run(dpf, dev, h, begin, db, W, stream=None):
    import torch
    K = dev.num_keys
    _dirty_scratch(dpf, dev, h)
    out = torch.full((max(K * W, 1) * 8,), POISON, dtype=torch.uint8, device="cuda")
    assert dpf.evaluate_dot_buckets_to_device(dev, h, begin, db, W, out[:K * W * 8]) == K * W
    torch.cuda.synchronize()
    return out.cpu().numpy()[:K * W * 8].view(np.uint64).reshape(K, W)


@functools.lru_cache(maxsize=None)
def _api_case(vt):
    """20 keys of both parties in 6 buckets ([0, 1, 17, 0, 1, 1]) of 2^7 rows."""
    n, W = 7, 3
    begin = [0, 0, 1, 18, 18, 19, 20]
    K, B = begin[-1], len(begin) - 1
    dpf = make([(n, vt, 0)])
    rng = np.random.default_rng(70 + (vt[0] == "xor"))
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=K)]
    alphas[:3] = [0, (1 << n) - 1, 1]
    betas = [_beta(k) for k in range(K)]
    host = dpf.generate_key_batch_with_betas(alphas, [leaves_value(vt, [b]) for b in betas],
                                             root_seeds=seeds_array(rng, K))
    db = rng.integers(0, 1 << 64, size=(B, 1 << n, W), dtype=np.uint64)
    return dpf, host, alphas, betas, begin, db, n, W


@pytest.mark.parametrize("vt", TYPES, ids=str)
def test_api_equals_evaluate_dot_key_by_key_and_reconstructs(vt):
    dpf, host, alphas, betas, begin, db, n, W = _api_case(vt)
    assert dpf.evaluates_dot_buckets_on_device(0)
    xor = vt[0] == "xor"
    ddb = _dev(db)
    bk = bucket_of_keys(begin)
    shares = []
    for party in (0, 1):
        dev = dpf.upload_key_batch(host[party])
        got = _run(dpf, dev, 0, begin, ddb, W)
        for k in range(len(alphas)):
            want = dpf.evaluate_dot(dpf.key_from_batch(host[party], k), 0, _dev(db[bk[k]]), W)
            assert got[k].tobytes() == np.ascontiguousarray(want).tobytes(), (party, k)
        np.testing.assert_array_equal(dpf.evaluate_dot_buckets(dev, 0, begin, ddb, W), got)
        shares.append(got)
    total = pir.reconstruct(shares[0], shares[1], xor)
    for k, (a, b) in enumerate(zip(alphas, betas)):
        rec = db[bk[k], a]
        np.testing.assert_array_equal(total[k], (np.uint64(b) & rec) if xor else np.uint64(b) * rec)


@pytest.mark.parametrize("chunk", [1, 3, 20])
def test_chunked_keys_give_equal_bytes(chunk, monkeypatch):
    """DPF_DOT_BUCKETS_CHUNK_KEYS in {1, 3, K}: the bucket of 17 keys is
    split across chunks."""
    vt = ("int", 64)
    dpf, host, alphas, betas, begin, db, n, W = _api_case(vt)
    dev = dpf.upload_key_batch(host[1])
    monkeypatch.delenv("DPF_DOT_BUCKETS_CHUNK_KEYS", raising=False)
    whole = _run(dpf, dev, 0, begin, _dev(db), W)
    monkeypatch.setenv("DPF_DOT_BUCKETS_CHUNK_KEYS", str(chunk))
    assert _run(dpf, dev, 0, begin, _dev(db), W).tobytes() == whole.tobytes()


def test_empty_batch_writes_nothing():
    import torch
    vt = ("int", 64)
    dpf, host, alphas, betas, begin, db, n, W = _api_case(vt)
    empty = dpf.upload_key_batch(host[0], 0, 0)
    out = torch.full((8,), POISON, dtype=torch.uint8, device="cuda")
    zeros = [0] * len(begin)
    assert dpf.evaluate_dot_buckets_to_device(empty, 0, zeros, _dev(db), W, out) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
    assert dpf.evaluate_dot_buckets(empty, 0, zeros, _dev(db), W).shape == (0, W)


def test_second_level_of_a_hierarchy_matches_the_oracle():
    vt = ("int", 64)
    levels = [(4, vt, 0), (9, vt, 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    n, W, K = 9, 2, 5
    begin = [0, 2, 2, 5]
    rng = np.random.default_rng(41)
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=K)]
    seeds = seeds_array(rng, K)
    betas = [[11], [13]]
    host = dpf.generate_key_batch(alphas, [leaves_value(vt, b) for b in betas], root_seeds=seeds)
    db = rng.integers(0, 1 << 64, size=(3, 1 << n, W), dtype=np.uint64)
    shares = []
    for party in (0, 1):
        got = _run(dpf, dpf.upload_key_batch(host[party]), 1, begin, _dev(db), W)
        ys = []
        for k in range(K):
            okey = O.generate_keys(P, alphas[k], betas, *seed_ints(seeds, k))[party]
            y = O.evaluate_until(P, 1, [], O.create_context(P, okey))
            ys.append(np.ascontiguousarray(y).view(np.uint64).reshape(1 << n))
        np.testing.assert_array_equal(got, dot_buckets(np.stack(ys), begin, db, False))
        shares.append(got)
    total = pir.reconstruct(shares[0], shares[1], False)
    bk = bucket_of_keys(begin)
    for k in range(K):
        np.testing.assert_array_equal(total[k], np.uint64(13) * db[bk[k], alphas[k]])


@pytest.mark.parametrize("two_streams", [False, True], ids=["one-stream", "two-streams"])
def test_two_calls_queued_back_to_back_are_both_right(two_streams):
    """Different keys, one scratch, no synchronise in between."""
    import torch
    vt = ("int", 64)
    dpf, host, alphas, betas, begin, db, n, W = _api_case(vt)
    ddb = _dev(db)
    devs = [dpf.upload_key_batch(host[p]) for p in (0, 1)]
    want = [_run(dpf, d, 0, begin, ddb, W) for d in devs]
    K = devs[0].num_keys
    outs = [torch.full((K * W,), -1, dtype=torch.int64, device="cuda") for _ in devs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream() if two_streams else None]
    streams[1] = streams[1] or streams[0]
    torch.cuda.synchronize()
    for d, o, s in zip(devs, outs, streams):
        dpf.evaluate_dot_buckets_to_device(d, 0, begin, ddb, W, o, stream=s)
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert o.cpu().numpy().view(np.uint64).tobytes() == w.tobytes()


# ---- the protocol -------------------------------------------------------------------
LAYOUT_SEED = 7      # tests/test_pir_buckets_cpu.py asserts that the schedule succeeds


def protocol_rows():
    return [int(r) for r in np.random.default_rng(16).choice(1 << 10, 16, replace=False)]


@pytest.mark.parametrize("vt", TYPES, ids=str)
def test_pir_buckets_end_to_end(vt):
    import torch
    R, B, W = 1 << 10, 24, 5
    xor = vt[0] == "xor"
    layout = pir.BucketLayout(R, B, LAYOUT_SEED)
    rows = protocol_rows()
    rng = np.random.default_rng(3)
    db = rng.integers(0, 1 << 64, size=(R, W), dtype=np.uint64)
    enc = _dev(layout.encode(db))
    dpf = make([(layout.log_bucket_size, vt, 0)])
    beta = MASK64 if xor else 1
    k0, k1, plan = pir.query_buckets(dpf, layout, rows, beta=beta)
    a0 = pir.answer_buckets(dpf, dpf.upload_key_batch(k0), layout, enc, W)
    a1 = pir.answer_buckets(dpf, dpf.upload_key_batch(k1), list(range(B + 1)), enc, W)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(pir.reconstruct_buckets(plan, a0, a1, xor), db[rows])


# ---- the calls that share the scratch -------------------------------------------------
def test_dot_batch_and_lookup_are_unchanged_after_the_new_calls():
    vt = ("int", 64)
    dpf, host, alphas, betas, begin, db, n, W = _api_case(vt)
    dev = dpf.upload_key_batch(host[0])
    keys = [dpf.key_from_batch(host[0], k) for k in range(4)]
    flat = _dev(db[2])
    table = _dev(db[1, :, :1])
    off = np.arange(dev.num_keys, dtype=np.uint64)
    before = (dpf.evaluate_dot_batch(keys, 0, flat, W), dpf.evaluate_lookup_batch(dev, 0, off, table, 1))
    _run(dpf, dev, 0, begin, _dev(db), W)
    after = (dpf.evaluate_dot_batch(keys, 0, flat, W), dpf.evaluate_lookup_batch(dev, 0, off, table, 1))
    for b, a in zip(before, after):
        assert np.ascontiguousarray(b).tobytes() == np.ascontiguousarray(a).tobytes()
