"""The batch-code protocol of pir.py around the bucketed fold, without a GPU:
the NumPy model of the fold against Python integers, BucketLayout's hashing,
encoding and cuckoo schedule, and the whole protocol with the oracle's
EvaluateUntil as the server."""
import numpy as np
import pytest

import oracle as O
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import pir
from dot_buckets_model import bucket_of_keys, dot_buckets, expected_shape
from test_key_batch_cpu import make, seeds_array

MASK64 = (1 << 64) - 1


# ---- the model ------------------------------------------------------------------------
def test_model_on_a_hand_worked_case():
    """Three buckets of two rows and two words, populations 2, 0, 1."""
    begin = [0, 2, 2, 3]
    y = [[3, MASK64], [0, 1], [1 << 63, 2]]
    db = [[[5, 7], [11, 1 << 63]],            # bucket 0
          [[99, 98], [97, 96]],               # bucket 1: read by no key
          [[2, 3], [MASK64, 6]]]              # bucket 2
    assert list(bucket_of_keys(begin)) == [0, 0, 2]
    want_add, want_xor = [], []
    for k, b in enumerate([0, 0, 2]):
        want_add.append([sum(y[k][i] * db[b][i][w] for i in range(2)) & MASK64 for w in range(2)])
        want_xor.append([(y[k][0] & db[b][0][w]) ^ (y[k][1] & db[b][1][w]) for w in range(2)])
    # By hand: key 0 word 0 = 3 * 5 + (2^64 - 1) * 11 = 15 - 11 = 4 mod 2^64.
    assert want_add[0][0] == 4 and want_add[1] == [11, 1 << 63]
    assert want_add[2] == [(2 * MASK64) & MASK64, ((3 << 63) + 12) & MASK64]
    assert want_xor[0] == [(3 & 5) ^ 11, (3 & 7) ^ (1 << 63)]
    yy, dd = np.array(y, dtype=np.uint64), np.array(db, dtype=np.uint64)
    assert dot_buckets(yy, begin, dd, False).tolist() == want_add
    assert dot_buckets(yy, begin, dd, True).tolist() == want_xor
    assert expected_shape(begin, 2) == (2, 2, 1)
    assert expected_shape([0, 0, 1, 18, 18, 83, 84], 130) == (1 + 2 + 5 + 1, 16, 3)


# ---- the layout -----------------------------------------------------------------------
def test_candidates_are_distinct_deterministic_and_in_range():
    a, b = pir.BucketLayout(500, 7, 11), pir.BucketLayout(500, 7, 11)
    other = pir.BucketLayout(500, 7, 12)
    differ = 0
    for r in range(500):
        c = a.candidates(r)
        assert len(c) == 3 and len(set(c)) == 3 and all(0 <= x < 7 for x in c)
        assert c == b.candidates(r)
        differ += c != other.candidates(r)
    assert differ > 250                       # another seed, another layout
    # choices == num_buckets: every bucket is a candidate of every row.
    full = pir.BucketLayout(20, 3, 1)
    assert all(sorted(full.candidates(r)) == [0, 1, 2] for r in range(20))
    assert len(pir.BucketLayout(50, 9, 2, choices=2).candidates(7)) == 2
    for bad in ((0, 5, 1), (10, 2, 1)):
        with pytest.raises(ValueError):
            pir.BucketLayout(*bad)


def test_position_is_the_rank_among_the_bucket_s_rows():
    L = pir.BucketLayout(300, 10, 5)
    members = {b: [r for r in range(300) if b in L.candidates(r)] for b in range(10)}
    assert sum(len(m) for m in members.values()) == 900
    for b, rows in members.items():
        assert [L.position(r, b) for r in rows] == list(range(len(rows)))
        assert L.loads[b] == len(rows)
    largest = max(len(m) for m in members.values())
    assert 1 << L.log_bucket_size >= largest
    assert L.log_bucket_size == 1 or 1 << (L.log_bucket_size - 1) < largest
    outsider = next(b for b in range(10) if b not in L.candidates(0))
    with pytest.raises(ValueError):
        L.position(0, outsider)
    assert pir.BucketLayout(1, 3, 0).log_bucket_size == 1     # n >= 1 whatever the load


def test_encode_places_every_record_at_its_positions_and_zero_elsewhere():
    R, B, W = 200, 9, 3
    L = pir.BucketLayout(R, B, 21)
    rng = np.random.default_rng(0)
    db = rng.integers(1, 1 << 64, size=(R, W), dtype=np.uint64)      # no zero record
    enc = L.encode(db)
    assert enc.shape == (B, 1 << L.log_bucket_size, W) and enc.dtype == np.uint64
    seen = np.zeros(enc.shape[:2], dtype=bool)
    for r in range(R):
        for b in L.candidates(r):
            p = L.position(r, b)
            assert not seen[b, p]
            seen[b, p] = True
            assert (enc[b, p] == db[r]).all()
    assert seen.sum() == 3 * R
    assert (enc[~seen] == 0).all()


# The layouts and rows of tests/test_dot_buckets_gpu.py's protocol test: their
# placement is asserted here, so that test cannot hide a failure of schedule().
def gpu_protocol_rows():
    return [int(r) for r in np.random.default_rng(16).choice(1 << 10, 16, replace=False)]


def test_schedule_succeeds_for_the_seeds_of_the_gpu_test():
    L = pir.BucketLayout(1 << 10, 24, 7)
    rows = gpu_protocol_rows()
    assert len(set(rows)) == 16
    buckets = L.schedule(rows)
    assert len(set(buckets)) == 16
    assert all(b in L.candidates(r) for r, b in zip(rows, buckets))
    assert buckets == L.schedule(rows)        # a pure function


def test_schedule_evicts_and_fails_cleanly():
    L = pir.BucketLayout(64, 3, 4)            # every row has all three buckets
    assert sorted(L.schedule([5, 9, 60])) == [0, 1, 2]
    with pytest.raises(ValueError, match="more rows than buckets"):
        L.schedule([1, 2, 3, 4])
    with pytest.raises(ValueError, match="distinct"):
        L.schedule([1, 1])
    with pytest.raises(ValueError, match="range"):
        L.schedule([64])
    # Full occupancy of a larger layout takes evictions; a placement it finds
    # is a valid one, and one it does not find raises.
    M = pir.BucketLayout(400, 12, 9)
    rows = [int(r) for r in np.random.default_rng(1).choice(400, 12, replace=False)]
    try:
        got = M.schedule(rows)
    except ValueError as e:
        assert "placement" in str(e)
    else:
        assert len(set(got)) == 12 and all(b in M.candidates(r) for r, b in zip(rows, got))


# ---- the protocol, the oracle as the server -------------------------------------------
def _oracle_key(key):
    """The oracle's key dictionary of a single-level DpfKey proto."""
    cws = [((cw.seed.high << 64) | cw.seed.low, int(cw.control_left), int(cw.control_right), None)
           for cw in key.correction_words]
    last = [[D._get_integer(getattr(v, v.WhichOneof("value")))]
            for v in key.last_level_value_correction]
    return {"seed": (key.seed.high << 64) | key.seed.low, "party": key.party, "cws": cws,
            "last_vc": last}


def _serve(dpf, P, batch, layout, enc, xor):
    """One server on the CPU: every bucket's key expanded by the oracle and
    folded into the bucket's slice by the model."""
    N = 1 << layout.log_bucket_size
    ys = []
    for b in range(layout.num_buckets):
        okey = _oracle_key(dpf.key_from_batch(batch, b))
        y = O.evaluate_until(P, 0, [], O.create_context(P, okey))
        ys.append(np.ascontiguousarray(y).view(np.uint64).reshape(N))
    return dot_buckets(np.stack(ys), list(range(layout.num_buckets + 1)), enc, xor)


@pytest.mark.parametrize("vt", [("int", 64), ("xor", 64)], ids=str)
def test_protocol_on_the_cpu_returns_beta_times_the_records(vt):
    R, B, W, Q = 60, 9, 3, 6
    xor = vt[0] == "xor"
    layout = pir.BucketLayout(R, B, 33)
    assert layout.log_bucket_size <= 6
    rng = np.random.default_rng(12)
    db = rng.integers(0, 1 << 64, size=(R, W), dtype=np.uint64)
    enc = layout.encode(db)
    levels = [(layout.log_bucket_size, vt, 0)]
    dpf, P = make(levels), O.OracleParams(levels)
    rows = [int(r) for r in rng.choice(R, Q, replace=False)]
    betas = [int(b) | 1 for b in rng.integers(1, 1 << 63, size=Q)]
    k0, k1, plan = pir.query_buckets(dpf, layout, rows, beta=betas,
                                     root_seeds=seeds_array(rng, B))
    assert k0.num_keys == k1.num_keys == B and plan.rows == rows
    assert all(b in layout.candidates(r) for r, b in zip(plan.rows, plan.buckets))
    a0 = _serve(dpf, P, k0, layout, enc, xor)
    a1 = _serve(dpf, P, k1, layout, enc, xor)
    got = pir.reconstruct_buckets(plan, a0, a1, xor)
    beta = np.array(betas, dtype=np.uint64)[:, None]
    np.testing.assert_array_equal(got, (beta & db[rows]) if xor else beta * db[rows])
    # The unused buckets answer zero: their keys are (0, 0).
    unused = sorted(set(range(B)) - set(plan.buckets))
    assert len(unused) == B - Q
    assert (pir.reconstruct(a0, a1, xor)[unused] == 0).all()
    # One beta for every row.
    k0, k1, plan = pir.query_buckets(dpf, layout, rows, beta=1 if not xor else MASK64)
    got = pir.reconstruct_buckets(plan, _serve(dpf, P, k0, layout, enc, xor),
                                  _serve(dpf, P, k1, layout, enc, xor), xor)
    np.testing.assert_array_equal(got, db[rows])


def test_query_buckets_rejects_a_dpf_of_another_domain():
    layout = pir.BucketLayout(60, 9, 33)
    with pytest.raises(ValueError):
        pir.query_buckets(make([(layout.log_bucket_size + 1, ("int", 64), 0)]), layout, [1, 2])
    with pytest.raises(ValueError):
        pir.query_buckets(make([(layout.log_bucket_size, ("int", 64), 0)]), layout, [1, 2],
                          beta=[1])
