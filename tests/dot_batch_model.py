"""NumPy model of the batched database fold (include/dpf_hip.h,
dpf_hip_dot_rows_batch):

    uint64_t:              out[q][w] = sum_i  y[q][i] * db[i][w]   (mod 2^64)
    XorWrapper<uint64_t>:  out[q][w] = XOR_i (y[q][i] & db[i][w])

np.uint64 products and sums wrap mod 2^64, which is the arithmetic wanted;
fold_ints takes the same sums in Python integers, where nothing wraps, and
reduces at the end (tests/test_dot_batch_cpu.py checks one against the other
and both against a hand-worked case).
"""
import numpy as np

MASK = (1 << 64) - 1


def fold(y, db, xor: bool) -> np.ndarray:
    """y (Q, n) uint64, db (n, W) uint64 -> (Q, W) uint64."""
    y = np.ascontiguousarray(y, dtype=np.uint64)
    db = np.ascontiguousarray(db, dtype=np.uint64)
    Q, n = y.shape
    out = np.zeros((Q, db.shape[1]), dtype=np.uint64)
    step = 1 << 12                       # rows per piece: (step, W) temporaries
    with np.errstate(over="ignore"):
        for q in range(Q):
            for i in range(0, n, step):
                yy = y[q, i:i + step, None]
                d = db[i:i + step]
                if xor:
                    out[q] ^= np.bitwise_xor.reduce(yy & d, axis=0)
                else:
                    out[q] += (yy * d).sum(axis=0, dtype=np.uint64)
    return out


def fold_ints(y, db, xor: bool) -> np.ndarray:
    """The same map in Python integers (small shapes only)."""
    Q, n, W = len(y), len(db), len(db[0]) if len(db) else 0
    out = np.zeros((Q, W), dtype=np.uint64)
    for q in range(Q):
        for w in range(W):
            a = 0
            for i in range(n):
                a = a ^ (int(y[q][i]) & int(db[i][w])) if xor else a + int(y[q][i]) * int(db[i][w])
            out[q, w] = a & MASK
    return out


def combine(a, b, xor: bool) -> np.ndarray:
    """T's + on uint64 arrays."""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return a ^ b if xor else a + b
