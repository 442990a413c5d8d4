"""Additive-share PIR batched over queries on the GPU: the word-weighted
database fold (dpf_hip_dot_rows_batch, EvaluateDotBatchToDevice, pir).

Reference: tests/dot_batch_model.py (np.uint64 wraparound, checked against
Python integers in tests/test_dot_batch_cpu.py) over seeded full-width random
shares and databases; for the API tests the shares are the CPU oracle's
EvaluateUntil outputs.  Sums mod 2^64 and XOR are exact in any order, so every
comparison is an equality.  After each kernel call the path and the number of
passes over the database are asserted: Q sequential passes must not pass for a
batched one.
"""
import functools

import numpy as np
import pytest

import dot_batch_model as M
import oracle as O

pytestmark = pytest.mark.gpu

U64, X64 = ("int", 64), ("xor", 64)
MAX_TILE = 16          # queries one pass over the database serves
MAX_GROUPS = 1024      # workgroups of one pass, as for dot_rows
POISON = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def hip():
    import torch
    from distributed_point_functions_amd import hip_abi
    hip_abi.load(require_gpu=True)
    assert torch.cuda.is_available()
    return hip_abi


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    for name in ("DPF_DOT_BATCH_SLAB_LOG", "DPF_DOT_BATCH_TILE", "DPF_DOT_SLAB_LOG",
                 "DPF_DOT_STREAM"):
        monkeypatch.delenv(name, raising=False)


def _is_xor(vt):
    return vt[0] == "xor"


def _desc(hip, vt):
    return hip.value_desc(O.leaves(vt), True, O.elements_per_block(vt), 1)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _tile(q):
    t = 1
    while t < min(q, MAX_TILE):
        t *= 2
    return t


# ------------------------------------------------------------- kernel alone
def _kernel_case(hip, vt, num_rows, W, Q, extra_stride=0, ones=False):
    import torch
    xor = _is_xor(vt)
    rng = np.random.default_rng(1 + 7 * num_rows + 31 * W + 131 * Q + xor)
    stride = max((num_rows * 8 + 15) // 16 * 16 + extra_stride, 16)
    # Every word random: the elements past num_rows and the padding must not count.
    y = rng.integers(0, 2**64, size=(Q, stride // 8), dtype=np.uint64)
    db = rng.integers(0, 2**64, size=(max(num_rows, 1), W), dtype=np.uint64)
    if ones:
        y[:, :num_rows] = np.uint64(2**64 - 1)
        db[:] = np.uint64(2**64 - 1)
    want = M.fold(y[:, :num_rows], db[:num_rows], xor)
    d_y = torch.from_numpy(y.view(np.int64)).cuda()
    d_db = torch.from_numpy(db.view(np.int64)).cuda()
    desc = _desc(hip, vt)
    # accumulate = 0 onto a poisoned output with a guard behind it.
    buf = torch.full((Q * W + 32,), POISON, dtype=torch.int64, device="cuda")
    ws = torch.full((hip.dot_batch_workspace_bytes(desc, W, Q),), 0xA5, dtype=torch.uint8,
                    device="cuda")
    hip.dot_rows_batch(num_rows, W, Q, desc, d_y, stride, d_db, workspace=ws, out=buf[:Q * W])
    torch.cuda.synchronize()
    assert hip.last_dot_kernel() == "rows_batch"
    tile, passes, groups = hip.last_dot_batch_shape()
    assert tile == _tile(Q) and passes == -(-Q // tile), (tile, passes, Q)
    got = _u64(buf[:Q * W]).reshape(Q, W)
    assert np.array_equal(got, want), (vt, num_rows, W, Q)
    assert bool((buf[Q * W:] == POISON).all())
    # accumulate = 1 onto a known output.
    known = rng.integers(0, 2**64, size=(Q, W), dtype=np.uint64)
    buf[:Q * W] = torch.from_numpy(known.view(np.int64).reshape(-1)).cuda()
    hip.dot_rows_batch(num_rows, W, Q, desc, d_y, stride, d_db, accumulate=True, workspace=ws,
                       out=buf[:Q * W])
    torch.cuda.synchronize()
    assert hip.last_dot_kernel() == "rows_batch"
    assert hip.last_dot_batch_shape()[1] == -(-Q // tile)
    assert np.array_equal(_u64(buf[:Q * W]).reshape(Q, W), M.combine(known, want, xor)), \
        (vt, num_rows, W, Q)
    assert bool((buf[Q * W:] == POISON).all())
    return groups, want


BIG = (1 << 15) + 77


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
@pytest.mark.parametrize("num_rows,W,Q", [
    (0, 3, 2), (1, 1, 1), (1, 33, 7), (63, 5, 7), (64, 2, 16), (65, 33, 17), (127, 257, 2),
    (129, 3, 64), (1000, 1024, 17), (1000, 5, 64),
    # A tile boundary, the last smaller pass, column chunks, narrow records, a ragged tail.
    (BIG, 1, 64), (BIG, 2, 7), (BIG, 5, 17), (BIG, 32, 16), (BIG, 257, 2),
], ids=str)
def test_dot_rows_batch(hip, vt, num_rows, W, Q):
    _kernel_case(hip, vt, num_rows, W, Q)


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
def test_dot_rows_batch_grid_over_the_workgroup_cap(hip, vt):
    num_rows, W, Q = (1 << 19) + 5, 3, 2
    # 256 rows per workgroup: more than 1024 workgroups are asked for.
    assert -(-num_rows // 256) > MAX_GROUPS
    assert _kernel_case(hip, vt, num_rows, W, Q)[0] == MAX_GROUPS


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
@pytest.mark.parametrize("num_rows,W,Q,extra", [(1000, 3, 17, 48), (129, 33, 2, 16)], ids=str)
def test_dot_rows_batch_larger_stride(hip, vt, num_rows, W, Q, extra):
    _kernel_case(hip, vt, num_rows, W, Q, extra_stride=extra)


def test_dot_rows_batch_all_ones_carries(hip):
    # (2^64 - 1)^2 = 1 mod 2^64, through every cross term: the sum is the row count.
    num_rows, W, Q = 1000, 5, 3
    _, want = _kernel_case(hip, U64, num_rows, W, Q, ones=True)
    assert np.array_equal(want, np.full((Q, W), num_rows, dtype=np.uint64))


def test_dot_rows_batch_wide_records_share_the_cap(hip):
    # 16 column chunks of 64 words: 64 workgroups along the rows, 1024 in all.
    assert _kernel_case(hip, U64, 20000, 1024, 1)[0] == MAX_GROUPS


# -------------------------------------------------------------------- API
MAXQ = 64


def _pvt(vt):
    from distributed_point_functions_amd import dpf as D
    return D.xor_wrapper_type(64) if _is_xor(vt) else D.integer_type(64)


@functools.lru_cache(maxsize=None)
def _queries(vt, depth):
    """64 key pairs with full-width betas; the first Q of them are a call's."""
    ld = depth + 1                       # a block holds two 64-bit elements
    P = O.OracleParams([(ld, vt, 0)])
    rng = np.random.default_rng(7000 + 100 * depth + _is_xor(vt))
    alphas = [int(a) for a in rng.choice(1 << ld, size=MAXQ, replace=False)]
    alphas[1] = alphas[0]                # two queries for the same record
    betas = [int(b) | 1 for b in rng.integers(0, 2**64, size=MAXQ, dtype=np.uint64)]
    seeds = [(0xB000 + 2 * q + 1000 * depth, 0xB001 + 2 * q + 1000 * depth) for q in range(MAXQ)]
    keys = [O.generate_keys(P, a, [[b]], s0, s1) for a, b, (s0, s1) in zip(alphas, betas, seeds)]
    return P, alphas, betas, seeds, keys


@functools.lru_cache(maxsize=4)
def _db(depth, W):
    rng = np.random.default_rng(199 + 31 * depth + W)
    return rng.integers(0, 2**64, size=(2 << depth, W), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _shares(vt, depth, party):
    """The oracle's EvaluateUntil outputs of the 64 keys, (64, n) uint64."""
    P, _, _, _, keys = _queries(vt, depth)
    rows = [np.ascontiguousarray(O.evaluate_until(P, 0, [], O.create_context(P, k[party])))
            .reshape(-1).view(np.uint64) for k in keys]
    assert all(r.size == 2 << depth for r in rows)
    return np.stack(rows)


@functools.lru_cache(maxsize=8)
def _reference(vt, depth, W, party):
    return M.fold(_shares(vt, depth, party), _db(depth, W), _is_xor(vt))


def _expected(vt, depth, W):
    """What the two parties' rows combine to: beta * db[alpha] (beta & db[alpha])."""
    _, alphas, betas, _, _ = _queries(vt, depth)
    db = _db(depth, W)
    out = np.zeros((MAXQ, W), dtype=np.uint64)
    for q, (a, b) in enumerate(zip(alphas, betas)):
        out[q] = [(b & int(d)) if _is_xor(vt) else (b * int(d)) & M.MASK for d in db[a]]
    return out


@functools.lru_cache(maxsize=None)
def _host(vt, depth):
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import proto as pb
    pvt = _pvt(vt)
    p = pb.DpfParameters(log_domain_size=depth + 1)
    p.value_type.CopyFrom(pvt)
    dpf = D.DistributedPointFunction.create(p)
    dpf.register_value_type(pvt)
    _, alphas, betas, seeds, _ = _queries(vt, depth)
    pairs = [dpf.generate_keys_incremental(a, [D.to_value(pvt, b)], seeds=s)
             for a, b, s in zip(alphas, betas, seeds)]
    return dpf, ([k[0] for k in pairs], [k[1] for k in pairs])


def _device_db(depth, W):
    import torch
    return torch.from_numpy(_db(depth, W).view(np.int64)).cuda()


def _host_batch(dpf, keys, db, W, shard=0, num_shards=1):
    import torch
    Q = len(keys)
    out = torch.full((Q * W + 16,), POISON, dtype=torch.int64, device="cuda")
    n = dpf.evaluate_dot_batch_to_device(keys, 0, db, W, out[:Q * W], shard=shard,
                                         num_shards=num_shards)
    torch.cuda.synchronize()
    assert n == Q * W
    assert bool((out[Q * W:] == POISON).all())
    return _u64(out[:Q * W]).reshape(Q, W)


def _host_tile(W):
    """Keys the host hands the kernel at a time."""
    return 8 if W >= 16 else 4


def _last_api_shape(Q, W):
    """(tile, passes) of the last kernel call of an API call with Q keys: the
    host hands the kernel _host_tile(W) keys at a time, one pass each, so Q
    keys cost ceil(Q / _host_tile(W)) passes over the database."""
    T = _host_tile(W)
    last = Q - (Q - 1) // T * T
    return (_tile(last), 1)


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
@pytest.mark.parametrize("depth", [7, 8, 9, 10, 11, 12])
def test_evaluate_dot_batch(hip, vt, depth):
    dpf, keys = _host(vt, depth)
    xor = _is_xor(vt)
    for W in (1, 3, 32, 65):
        db = _device_db(depth, W)
        # What EvaluateDotToDevice writes for each key on its own.
        single = [np.stack([np.asarray(dpf.evaluate_dot(k, 0, db, W)).reshape(W)
                            for k in keys[party]]) for party in (0, 1)]
        for Q in (1, 3, 16, 17, 64):
            got = []
            for party in (0, 1):
                got.append(_host_batch(dpf, keys[party][:Q], db, W))
                assert hip.last_dot_kernel() == "rows_batch"
                assert hip.last_dot_batch_shape()[:2] == _last_api_shape(Q, W)
                assert np.array_equal(got[-1], single[party][:Q]), (vt, depth, W, Q, party)
                assert np.array_equal(got[-1], _reference(vt, depth, W, party)[:Q]), \
                    (vt, depth, W, Q, party)
            assert np.array_equal(M.combine(got[0], got[1], xor), _expected(vt, depth, W)[:Q])


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
def test_eight_slabs_equal_the_unslabbed_answer(hip, monkeypatch, vt):
    depth, Q, W = 10, 5, 3               # 2048 records
    dpf, keys = _host(vt, depth)
    db = _device_db(depth, W)
    whole = _host_batch(dpf, keys[0][:Q], db, W)
    groups_whole = hip.last_dot_batch_shape()[2]
    monkeypatch.setenv("DPF_DOT_BATCH_SLAB_LOG", "8")
    slabbed = _host_batch(dpf, keys[0][:Q], db, W)
    # 2048 records in eight slabs of 256: one workgroup of 256 rows, not eight.
    assert (groups_whole, hip.last_dot_batch_shape()[2]) == (8, 1)
    assert np.array_equal(slabbed, whole)
    assert np.array_equal(whole, _reference(vt, depth, W, 0)[:Q])
    # The hook is clamped to one leaf block (two records).
    monkeypatch.setenv("DPF_DOT_BATCH_SLAB_LOG", "0")
    dpf7, keys7 = _host(vt, 7)
    assert np.array_equal(_host_batch(dpf7, keys7[0][:Q], _device_db(7, W), W),
                          _reference(vt, 7, W, 0)[:Q])


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
def test_host_tiles_equal_the_whole_call(hip, monkeypatch, vt):
    # 17 keys a tile of 2 at a time (the last tile holds one), with slabs.
    depth, Q, W = 9, 17, 3
    dpf, keys = _host(vt, depth)
    db = _device_db(depth, W)
    monkeypatch.setenv("DPF_DOT_BATCH_TILE", "2")
    monkeypatch.setenv("DPF_DOT_BATCH_SLAB_LOG", "8")
    got = _host_batch(dpf, keys[1][:Q], db, W)
    assert hip.last_dot_batch_shape() == (1, 1, 1)
    assert np.array_equal(got, _reference(vt, depth, W, 1)[:Q])


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
@pytest.mark.parametrize("num_shards", [2, 4])
def test_shards_combine_to_the_unsharded_answer(hip, vt, num_shards):
    from distributed_point_functions_amd import dpf as D
    depth, Q, W = 9, 5, 3
    dpf, keys = _host(vt, depth)
    db = _device_db(depth, W)
    rows = db.shape[0] // num_shards
    for party in (0, 1):
        total = np.zeros((Q, W), dtype=np.uint64)
        for shard in range(num_shards):
            total = M.combine(total, _host_batch(
                dpf, keys[party][:Q], db[shard * rows:(shard + 1) * rows].contiguous(), W,
                shard=shard, num_shards=num_shards), _is_xor(vt))
        assert np.array_equal(total, _reference(vt, depth, W, party)[:Q])
    with pytest.raises(D.DpfStatusError) as e:
        _host_batch(dpf, keys[0][:Q], db, W, shard=0, num_shards=1 << (depth + 1))
    assert e.value.code == 3 and "more shards" in e.value.message


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
def test_two_shards_of_four_slabs_each(hip, monkeypatch, vt):
    # 2048 records: each shard's 1024 in four slabs of 256, so the slab roots
    # lie at tree path (shard << 2) | slab and the correction words are cut there.
    depth, Q, W = 10, 5, 3
    monkeypatch.setenv("DPF_DOT_BATCH_SLAB_LOG", "8")
    dpf, keys = _host(vt, depth)
    db = _device_db(depth, W)
    rows = db.shape[0] // 2
    for party in (0, 1):
        total = np.zeros((Q, W), dtype=np.uint64)
        for shard in range(2):
            total = M.combine(total, _host_batch(
                dpf, keys[party][:Q], db[shard * rows:(shard + 1) * rows].contiguous(), W,
                shard=shard, num_shards=2), _is_xor(vt))
            assert hip.last_dot_batch_shape()[2] == 1    # workgroups of one slab's 256 rows
        assert np.array_equal(total, _reference(vt, depth, W, party)[:Q])


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
def test_python_evaluate_dot_batch(hip, vt):
    depth, Q, W = 9, 3, 4
    dpf, keys = _host(vt, depth)
    db = _device_db(depth, W)
    got = [dpf.evaluate_dot_batch(keys[p][:Q], 0, db, W) for p in (0, 1)]
    for party in (0, 1):
        assert got[party].dtype == np.uint64 and got[party].shape == (Q, W)
        assert np.array_equal(got[party], _reference(vt, depth, W, party)[:Q])
    assert np.array_equal(M.combine(got[0], got[1], _is_xor(vt)), _expected(vt, depth, W)[:Q])
    rows = db.shape[0] // 2
    halves = [dpf.evaluate_dot_batch(keys[0][:Q], 0, db[s * rows:(s + 1) * rows].contiguous(), W,
                                     shard=s, num_shards=2) for s in (0, 1)]
    assert np.array_equal(M.combine(halves[0], halves[1], _is_xor(vt)), got[0])


@pytest.mark.parametrize("vt", [U64, X64], ids=str)
def test_pir_end_to_end(hip, vt):
    """20 clients fetch 20 rows of a 2^10 x 48-word table."""
    import torch
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import pir
    from distributed_point_functions_amd import proto as pb
    pvt = _pvt(vt)
    p = pb.DpfParameters(log_domain_size=10)
    p.value_type.CopyFrom(pvt)
    dpf = D.DistributedPointFunction.create(p)
    dpf.register_value_type(pvt)
    rng = np.random.default_rng(2024)
    table = rng.integers(0, 2**64, size=(1 << 10, 48), dtype=np.uint64)
    rows = [int(r) for r in rng.integers(0, 1 << 10, size=20)]
    rows[3] = rows[2]
    seeds = [(0xC000 + 2 * i, 0xC001 + 2 * i) for i in range(20)]
    d_table = torch.from_numpy(table.view(np.int64)).cuda()
    # beta = 1 (all ones for XOR): the answer is the record itself.
    beta = M.MASK if _is_xor(vt) else 1
    k0, k1 = pir.query(dpf, rows, beta=beta, root_seeds=seeds)
    assert len(k0) == len(k1) == 20
    a0 = pir.answer(dpf, k0, d_table, 48)
    assert hip.last_dot_kernel() == "rows_batch"
    assert hip.last_dot_batch_shape()[:2] == _last_api_shape(20, 48) == (4, 1)
    a1 = pir.answer(dpf, k1, d_table, 48, out=torch.empty((20, 48), dtype=torch.int64,
                                                          device="cuda"))
    torch.cuda.synchronize()
    assert a0.shape == (20, 48)
    got = pir.reconstruct(a0, a1, xor=_is_xor(vt))
    assert np.array_equal(got, table[rows])
    # A weighted fetch: per-query betas, fresh randomness.
    betas = [int(b) for b in rng.integers(0, 2**64, size=20, dtype=np.uint64)]
    k0, k1 = pir.query(dpf, rows, beta=betas)
    got = pir.reconstruct(pir.answer(dpf, k0, d_table, 48), pir.answer(dpf, k1, d_table, 48),
                          xor=_is_xor(vt))
    want = np.array([[(b & int(d)) if _is_xor(vt) else (b * int(d)) & M.MASK for d in table[r]]
                     for r, b in zip(rows, betas)], dtype=np.uint64)
    assert np.array_equal(got, want)


def test_no_regression_in_dot_and_select(hip):
    """evaluate_dot and evaluate_select still give what the oracle gives."""
    depth, W = 7, 3
    dpf, keys = _host(U64, depth)
    db = _device_db(depth, W)
    got = np.asarray(dpf.evaluate_dot(keys[0][0], 0, db, W)).reshape(W)
    assert hip.last_dot_kernel() == "rows"
    assert np.array_equal(got, _reference(U64, depth, W, 0)[0])
    # The bit-selected fold: one record per output bit, 64 per element.
    xdpf, xkeys = _host(X64, depth)
    rng = np.random.default_rng(5)
    import torch
    records = rng.integers(0, 2**64, size=((2 << depth) * 64, W), dtype=np.uint64)
    sel = dpf_bits = np.unpackbits(_shares(X64, depth, 0)[:2].view(np.uint8).reshape(2, -1),
                                   axis=1, bitorder="little").astype(bool)
    assert dpf_bits.shape == (2, records.shape[0])
    want = np.stack([np.bitwise_xor.reduce(records[sel[q]], axis=0, initial=np.uint64(0))
                     for q in range(2)])
    got = xdpf.evaluate_select(xkeys[0][:2], 0, torch.from_numpy(records.view(np.int64)).cuda(), W)
    assert hip.last_dot_kernel() == "select"
    assert np.array_equal(got, want)
