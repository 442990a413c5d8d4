"""Python-int model of the per-key linear sketch (include/dpf_hip.h,
dpf_hip_sketch_rows) over packed oracle outputs:

    sketch[k][j][e] = ( sum_i (w[j][i] mod N_e) * y_k[i][e] ) mod N_e

for a value type whose leaves are all IntModN<uint32, N_e>.  The sums are
taken over numpy object arrays, i.e. in Python integers: nothing wraps.
"""
import numpy as np

import oracle as O


def moduli(vt):
    ls = O.leaves(vt)
    assert all(kind == O.LEAF_INTMODN and bits == 32 for kind, bits, _ in ls), vt
    return [int(m) for _, _, m in ls]


def sketch(vt, packed_rows, weights) -> np.ndarray:
    """packed_rows: uint8, K rows of n packed elements (any shape holding
    K * n * packed_size(vt) bytes, given K = len(packed_rows)); weights: J rows
    of n integers below 2^32.  Returns uint32 (K, J, nl)."""
    mods = moduli(vt)
    nl = len(mods)
    rows = np.ascontiguousarray(packed_rows, dtype=np.uint8)
    K = rows.shape[0]
    y = rows.reshape(K, -1).view("<u4").reshape(K, -1, nl).astype(object)
    w = np.asarray(weights, dtype=np.uint64).astype(object)
    J, n = w.shape
    assert y.shape[1] == n, (y.shape, w.shape)
    out = np.zeros((K, J, nl), dtype=np.uint32)
    for e, N in enumerate(mods):
        s = np.dot(w % N, y[:, :, e].T) if n else np.zeros((J, K), dtype=object)   # (J, K)
        out[:, :, e] = (s % N).T.astype(np.uint32)
    return out
