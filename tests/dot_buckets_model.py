"""NumPy model of the segmented fold of dpf_hip_dot_buckets: every key's share
row folded into its own bucket's slice of the database.  Sums mod 2^64 and XOR
are exact in any order, so the model is the definition written down."""
import numpy as np


def bucket_of_keys(bucket_begin):
    """b(k) for every key, from the B + 1 entries of bucket_begin."""
    bb = np.asarray(bucket_begin, dtype=np.int64)
    return np.repeat(np.arange(len(bb) - 1, dtype=np.int64), np.diff(bb))


def dot_buckets(y, bucket_begin, db, xor):
    """y: (K, N) uint64 shares; db: (B, N, W) uint64; returns (K, W) uint64:
    out[k][w] = sum_i y[k][i] * db[b(k)][i][w] mod 2^64, or XOR_i (y & db)."""
    y = np.asarray(y, dtype=np.uint64)
    db = np.asarray(db, dtype=np.uint64)
    K, W = y.shape[0], db.shape[2]
    out = np.zeros((K, W), dtype=np.uint64)
    for k, b in enumerate(bucket_of_keys(bucket_begin)):
        if xor:
            out[k] = np.bitwise_xor.reduce(y[k][:, None] & db[b], axis=0)
        else:
            with np.errstate(over="ignore"):
                out[k] = (y[k][:, None] * db[b]).sum(axis=0, dtype=np.uint64)
    return out


def expected_shape(bucket_begin, record_words):
    """(tiles, largest tile, column chunks) of a call: a bucket of p keys
    takes ceil(p / 16) tiles, an empty one none."""
    pops = np.diff(np.asarray(bucket_begin, dtype=np.int64))
    tiles = int(((pops + 15) // 16).sum())
    largest = int(min(16, pops.max())) if len(pops) else 0
    return tiles, largest, (int(record_words) + 63) // 64
