"""Dense PIR on the GPU: the bit-selected database fold batched over queries
(dpf_hip_select_rows, EvaluateSelectToDevice).

Reference: numpy.  Row q of the selection (for the API tests: the oracle's
EvaluateUntil output of key q, read as bytes) is unpacked little-endian, its
first num_rows bits select rows of a seeded random uint64 database, and
np.bitwise_xor.reduce folds them.  XOR commutes, so every comparison is an
equality.  After each kernel call the path and the number of passes over the
database are asserted: Q sequential passes must not pass for a batched one.
"""
import functools

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

X64, X128 = ("xor", 64), ("xor", 128)
MAX_TILE = 16          # queries one pass over the database serves
MAX_GROUPS = 1024      # workgroups of one pass, as for dot_rows


@pytest.fixture(scope="module")
def hip():
    import torch
    from distributed_point_functions_amd import hip_abi
    hip_abi.load(require_gpu=True)
    assert torch.cuda.is_available()
    return hip_abi


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    monkeypatch.delenv("DPF_SELECT_SLAB_LOG", raising=False)


def _fold(sel_rows, num_rows, db):
    """sel_rows (Q, bytes) uint8, db (rows, W) uint64 -> (Q, W) uint64."""
    out = np.zeros((sel_rows.shape[0], db.shape[1]), dtype=np.uint64)
    for q in range(sel_rows.shape[0]):
        bits = np.unpackbits(sel_rows[q], bitorder="little")[:num_rows]
        out[q] = np.bitwise_xor.reduce(db[:num_rows][bits.astype(bool)], axis=0,
                                       initial=np.uint64(0))
    return out


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _tile(q):
    t = 1
    while t < min(q, MAX_TILE):
        t *= 2
    return t


# ------------------------------------------------------------- kernel alone
def _kernel_case(hip, num_rows, W, Q, extra_stride=0, seed=0):
    import torch
    rng = np.random.default_rng(1 + 7 * num_rows + 31 * W + 131 * Q + seed)
    stride = (-(-num_rows // 8) + 15) // 16 * 16 + extra_stride
    stride = max(stride, 16)
    # Every byte random: the bits past num_rows and the padding must not count.
    sel = rng.integers(0, 256, size=(Q, stride), dtype=np.uint8)
    db = rng.integers(0, 2**64, size=(max(num_rows, 1), W), dtype=np.uint64)
    want = _fold(sel, num_rows, db)
    d_sel = torch.from_numpy(sel).cuda()
    d_db = torch.from_numpy(db.view(np.int64)).cuda()
    # accumulate = 0 onto a poisoned output with a guard behind it.
    buf = torch.full((Q * W + 32,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    ws = torch.full((hip.select_workspace_bytes(W, Q),), 0xA5, dtype=torch.uint8, device="cuda")
    hip.select_rows(num_rows, W, Q, d_sel, stride, d_db, workspace=ws, out=buf[:Q * W])
    torch.cuda.synchronize()
    assert hip.last_dot_kernel() == "select"
    tile, passes, groups = hip.last_select_shape()
    assert tile == _tile(Q) and passes == -(-Q // tile), (tile, passes, Q)
    got = _u64(buf[:Q * W]).reshape(Q, W)
    assert np.array_equal(got, want), (num_rows, W, Q)
    assert bool((buf[Q * W:] == 0x5A5A5A5A5A5A5A5A).all())
    # accumulate = 1 onto a known output.
    known = rng.integers(0, 2**64, size=(Q, W), dtype=np.uint64)
    buf[:Q * W] = torch.from_numpy(known.view(np.int64).reshape(-1)).cuda()
    hip.select_rows(num_rows, W, Q, d_sel, stride, d_db, accumulate=True, workspace=ws,
                    out=buf[:Q * W])
    torch.cuda.synchronize()
    assert hip.last_dot_kernel() == "select"
    assert hip.last_select_shape()[1] == -(-Q // tile)
    assert np.array_equal(_u64(buf[:Q * W]).reshape(Q, W), known ^ want), (num_rows, W, Q)
    assert bool((buf[Q * W:] == 0x5A5A5A5A5A5A5A5A).all())
    return groups


BIG = (1 << 15) + 77


@pytest.mark.parametrize("num_rows,W,Q", [
    (0, 3, 2), (0, 1, 17),
    (1, 1, 1), (1, 33, 7),
    (63, 5, 7), (63, 2, 1),
    (64, 2, 16), (64, 32, 2),
    (65, 33, 17), (65, 1, 2),
    (127, 257, 2), (127, 3, 16),
    (129, 3, 64), (129, 256, 1),
    (1000, 1024, 17), (1000, 256, 7), (1000, 33, 1), (1000, 5, 64),
    (BIG, 5, 17), (BIG, 32, 16), (BIG, 1, 64), (BIG, 2, 7), (BIG, 257, 2),
], ids=str)
def test_select_rows(hip, num_rows, W, Q):
    _kernel_case(hip, num_rows, W, Q)


@pytest.mark.parametrize("num_rows,W,Q", [
    ((1 << 19) + 5, 1, 3), ((1 << 18) + 3, 5, 2),
    # From 2 (8) groups of 64 rows per wave on, a wave takes 2 (8) consecutive
    # groups at a time; for W <= 2, 8 consecutive steps and not 4.
    ((1 << 19) + 5, 3, 2), ((1 << 21) + 70, 4, 5), ((1 << 21) + 70, 1, 3), ((1 << 21) + 70, 2, 2),
], ids=str)
def test_select_rows_grid_over_the_workgroup_cap(hip, num_rows, W, Q):
    # 256 rows per workgroup: all ask for more than 1024 workgroups.
    assert -(-num_rows // 256) > MAX_GROUPS
    assert _kernel_case(hip, num_rows, W, Q) == MAX_GROUPS


@pytest.mark.parametrize("num_rows,W,Q,extra", [(1000, 3, 17, 48), (129, 33, 2, 16)], ids=str)
def test_select_rows_larger_stride(hip, num_rows, W, Q, extra):
    _kernel_case(hip, num_rows, W, Q, extra_stride=extra)


def test_select_rows_wide_records_share_the_cap(hip):
    # 16 column chunks of 64 words: 64 workgroups along the rows, 1024 in all.
    assert _kernel_case(hip, 20000, 1024, 1) == MAX_GROUPS


# -------------------------------------------------------------------- API
def _bits(vt):
    return vt[1]


def _log_domain(vt, depth):
    """Tree depth -> log_domain_size: a uint64 block holds two elements."""
    return depth + 1 if vt[1] == 64 else depth


@functools.lru_cache(maxsize=None)
def _queries(vt, depth, Q, share_alpha=False):
    """Q key pairs: distinct alphas (or the first two equal), the first beta
    one bit -- a client asking for one record --, the others several bits."""
    ld = _log_domain(vt, depth)
    P = O.OracleParams([(ld, vt, 0)])
    rng = np.random.default_rng(5000 + 100 * depth + Q + vt[1] + share_alpha)
    alphas = [int(a) for a in rng.choice(1 << ld, size=Q, replace=False)]
    if share_alpha:
        alphas[1] = alphas[0]
    betas = [1 << int(rng.integers(0, vt[1]))]
    betas += [int.from_bytes(rng.bytes(vt[1] // 8), "little") | 5 for _ in range(Q - 1)]
    seeds = [(0xA000 + 2 * q + 1000 * depth, 0xA001 + 2 * q + 1000 * depth) for q in range(Q)]
    keys = [O.generate_keys(P, a, [[b]], s0, s1) for a, b, (s0, s1) in zip(alphas, betas, seeds)]
    return P, alphas, betas, seeds, keys


@functools.lru_cache(maxsize=4)
def _db(vt, depth, W):
    rng = np.random.default_rng(99 + 31 * depth + W + vt[1])
    return rng.integers(0, 2**64, size=((1 << depth) * 128, W), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _reference(vt, depth, Q, W, party, share_alpha=False):
    """The oracle's share vectors as bit rows, folded into the database."""
    P, _, _, _, keys = _queries(vt, depth, Q, share_alpha)
    rows = []
    for k in keys:
        y = O.evaluate_until(P, 0, [], O.create_context(P, k[party]))
        rows.append(np.ascontiguousarray(y).reshape(-1).view(np.uint8))
    n = (1 << depth) * 128
    assert all(r.size * 8 == n for r in rows)
    return _fold(np.stack(rows), n, _db(vt, depth, W))


def _selected(vt, depth, Q, W, share_alpha=False):
    """What the two parties' answers XOR to: the records beta's bits name."""
    _, alphas, betas, _, _ = _queries(vt, depth, Q, share_alpha)
    db, B = _db(vt, depth, W), _bits(vt)
    out = np.zeros((Q, W), dtype=np.uint64)
    for q, (a, b) in enumerate(zip(alphas, betas)):
        for bit in range(B):
            if (b >> bit) & 1:
                out[q] ^= db[a * B + bit]
    return out


def _host(vt, depth, Q, share_alpha=False):
    from distributed_point_functions_amd import dpf as D
    from distributed_point_functions_amd import proto as pb
    pvt = D.xor_wrapper_type(vt[1])
    p = pb.DpfParameters(log_domain_size=_log_domain(vt, depth))
    p.value_type.CopyFrom(pvt)
    dpf = D.DistributedPointFunction.create(p)
    dpf.register_value_type(pvt)
    _, alphas, betas, seeds, _ = _queries(vt, depth, Q, share_alpha)
    pairs = [dpf.generate_keys_incremental(a, [D.to_value(pvt, b)], seeds=s)
             for a, b, s in zip(alphas, betas, seeds)]
    return dpf, ([k[0] for k in pairs], [k[1] for k in pairs])


def _device_db(vt, depth, W):
    import torch
    return torch.from_numpy(_db(vt, depth, W).view(np.int64)).cuda()


def _host_select(dpf, keys, db, W, shard=0, num_shards=1):
    import torch
    Q = len(keys)
    out = torch.full((Q * W + 16,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    n = dpf.evaluate_select_to_device(keys, 0, db, W, out[:Q * W], shard=shard,
                                      num_shards=num_shards)
    torch.cuda.synchronize()
    assert n == Q * W
    assert bool((out[Q * W:] == 0x5A5A5A5A5A5A5A5A).all())
    return _u64(out[:Q * W]).reshape(Q, W)


@pytest.mark.parametrize("vt", [X64, X128], ids=str)
@pytest.mark.parametrize("depth,Q,W,share", [
    (0, 1, 4, False),      # one leaf block: 128 records
    (1, 2, 1, True),       # two queries for the same block
    (5, 3, 33, False),
    (5, 17, 1, False),     # two passes over the database
    (13, 3, 4, False),
    (13, 17, 1, True),
], ids=str)
def test_evaluate_select(hip, vt, depth, Q, W, share):
    dpf, keys = _host(vt, depth, Q, share)
    db = _device_db(vt, depth, W)
    got = []
    for party in (0, 1):
        got.append(_host_select(dpf, keys[party], db, W))
        assert hip.last_dot_kernel() == "select"
        assert hip.last_select_shape()[:2] == (_tile(Q), -(-Q // _tile(Q)))
        assert np.array_equal(got[-1], _reference(vt, depth, Q, W, party, share)), (vt, party)
    assert np.array_equal(got[0] ^ got[1], _selected(vt, depth, Q, W, share))


@pytest.mark.parametrize("vt", [X64, X128], ids=str)
def test_eight_slabs_equal_the_unslabbed_answer(hip, monkeypatch, vt):
    depth, Q, W = 5, 3, 4
    dpf, keys = _host(vt, depth, Q)
    db = _device_db(vt, depth, W)
    whole = _host_select(dpf, keys[0], db, W)
    groups_whole = hip.last_select_shape()[2]
    monkeypatch.setenv("DPF_SELECT_SLAB_LOG", "9")
    slabbed = _host_select(dpf, keys[0], db, W)
    # 4096 records in slabs of 512: two workgroups of 256 rows, not sixteen.
    assert (groups_whole, hip.last_select_shape()[2]) == (16, 2)
    assert np.array_equal(slabbed, whole)
    assert np.array_equal(whole, _reference(vt, depth, Q, W, 0))
    # The hook is clamped to one leaf block.
    monkeypatch.setenv("DPF_SELECT_SLAB_LOG", "0")
    assert np.array_equal(_host_select(dpf, keys[0], db, W), whole)
    assert hip.last_select_shape()[2] == 1


@pytest.mark.parametrize("vt", [X64, X128], ids=str)
@pytest.mark.parametrize("num_shards", [2, 4])
def test_shards_xor_to_the_unsharded_answer(hip, vt, num_shards):
    from distributed_point_functions_amd import dpf as D
    depth, Q, W = 5, 3, 4
    dpf, keys = _host(vt, depth, Q)
    db = _device_db(vt, depth, W)
    rows = db.shape[0] // num_shards
    for party in (0, 1):
        total = np.zeros((Q, W), dtype=np.uint64)
        for shard in range(num_shards):
            total ^= _host_select(dpf, keys[party], db[shard * rows:(shard + 1) * rows].contiguous(),
                                  W, shard=shard, num_shards=num_shards)
        assert np.array_equal(total, _reference(vt, depth, Q, W, party))
    with pytest.raises(D.DpfStatusError) as e:
        _host_select(dpf, keys[0], db, W, shard=0, num_shards=64)
    assert e.value.code == 3 and "more shards" in e.value.message


@pytest.mark.parametrize("vt", [X64, X128], ids=str)
def test_two_shards_of_four_slabs_each(hip, monkeypatch, vt):
    # 4096 records: each shard's 2048 in four slabs of 512, so the slab roots
    # lie at tree path (shard << 2) | slab and the correction words are cut there.
    depth, Q, W = 5, 3, 4
    monkeypatch.setenv("DPF_SELECT_SLAB_LOG", "9")
    dpf, keys = _host(vt, depth, Q)
    db = _device_db(vt, depth, W)
    rows = db.shape[0] // 2
    for party in (0, 1):
        total = np.zeros((Q, W), dtype=np.uint64)
        for shard in range(2):
            total ^= _host_select(dpf, keys[party], db[shard * rows:(shard + 1) * rows].contiguous(),
                                  W, shard=shard, num_shards=2)
            assert hip.last_select_shape()[2] == 2     # workgroups of one slab's 512 rows
        assert np.array_equal(total, _reference(vt, depth, Q, W, party))


@pytest.mark.parametrize("vt", [X64, X128], ids=str)
def test_python_evaluate_select(hip, vt):
    depth, Q, W = 5, 3, 4
    dpf, keys = _host(vt, depth, Q)
    db = _device_db(vt, depth, W)
    got = [dpf.evaluate_select(keys[p], 0, db, W) for p in (0, 1)]
    for party in (0, 1):
        assert got[party].dtype == np.uint64 and got[party].shape == (Q, W)
        assert np.array_equal(got[party], _reference(vt, depth, Q, W, party))
    assert np.array_equal(got[0] ^ got[1], _selected(vt, depth, Q, W))
    rows = db.shape[0] // 2
    halves = [dpf.evaluate_select(keys[0], 0, db[s * rows:(s + 1) * rows].contiguous(), W,
                                  shard=s, num_shards=2) for s in (0, 1)]
    assert np.array_equal(halves[0] ^ halves[1], got[0])
