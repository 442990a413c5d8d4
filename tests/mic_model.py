"""Python restatement of the multiple-interval-containment gate (eprint
2020/1392 Fig. 14; dcf/fss_gates/multiple_interval_containment.cc:104-275) over
the CPU oracle's DCF (oracle.dcf_generate_keys / oracle.dcf_evaluate with value
type uint128).  The tests compare the product's keys and outputs against it."""
import numpy as np

import oracle as O

VT = ("int", 128)


def params(n):
    return O.dcf_params(n, VT)


def gen(n, intervals, r_in, r_out, seed_0, seed_1, z_0):
    """Gen with the DCF's root seeds and party 0's mask shares given.  Returns
    two keys {"dcf": oracle DCF key, "shares": [z_i,b]}."""
    N = 1 << n
    assert len(r_out) == len(intervals) == len(z_0)
    d0, d1 = O.dcf_generate_keys(params(n), (N - 1 + r_in) % N, [1], seed_0, seed_1)
    s0, s1 = [], []
    for (p, q), ro, z0 in zip(intervals, r_out, z_0):
        qp = (q + 1) % N
        ap, aq, aqp = (p + r_in) % N, (q + r_in) % N, (q + 1 + r_in) % N
        z = (ro + (ap > aq) - (ap > p) + (aqp > qp) + (aq == N - 1)) % N
        s0.append(z0 % N)
        s1.append((z - z0) % N)
    return {"dcf": d0, "shares": s0}, {"dcf": d1, "shares": s1}


def dcf_value(n, dcf_key, x):
    return int.from_bytes(O.dcf_evaluate(params(n), dcf_key, x).tobytes(), "little")


def evaluate(n, intervals, key, x, cache=None):
    """Eval: one share per interval.  `cache` (a dict) keeps DCF values by point."""
    N = 1 << n
    cache = {} if cache is None else cache

    def dcf(pt):
        if pt not in cache:
            cache[pt] = dcf_value(n, key["dcf"], pt)
        return cache[pt]

    out = []
    for (p, q), z in zip(intervals, key["shares"]):
        qp = (q + 1) % N
        y = ((x > p) - (x > qp)) if key["dcf"]["party"] else 0
        y += -dcf((x + N - 1 - p) % N) + dcf((x + N - 1 - qp) % N) + z
        out.append(y % N)
    return out


def contains(intervals, x):
    return [1 if p <= x <= q else 0 for p, q in intervals]


def reconstruct(n, a, b, r_out):
    N = 1 << n
    return [(u + v - r) % N for u, v, r in zip(a, b, r_out)]


def partition(n, m):
    """m adjacent intervals that cover Z_{2^n}."""
    N = 1 << n
    cuts = [i * N // m for i in range(m)] + [N]
    return [(cuts[i], cuts[i + 1] - 1) for i in range(m)]


def disjoint(n, m, rng):
    """m non-adjacent intervals (a gap of at least 2 between neighbours, none
    touching 0 or N - 1): 2 m distinct offsets."""
    N = 1 << n
    width = N // (m + 1)
    assert width >= 8
    out = []
    for i in range(m):
        base = 1 + i * width
        lo = base + int.from_bytes(rng.bytes(16), "little") % (width // 4)
        hi = lo + int.from_bytes(rng.bytes(16), "little") % (width // 4)
        out.append((lo, hi))
    return out


def u128_rows(values):
    """Python ints -> uint64 (len, 2) {low, high}."""
    a = np.empty((len(values), 2), np.uint64)
    for i, v in enumerate(values):
        a[i, 0] = v & (2**64 - 1)
        a[i, 1] = v >> 64
    return a


def ints_of(a):
    a = np.asarray(a).view(np.uint64).reshape(-1, 2)
    return [(int(h) << 64) | int(l) for l, h in a]
