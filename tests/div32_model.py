"""Python-int restatement of the invariant-divisor arithmetic of
csrc/kernels/dpf_device.h (Div32, div_2by1, divmod128, mod32, mul_mod, mod64)
and of the tuple sampling built on it, with a census of the data-dependent
corrections each input takes.

The reference for RESULTS is always plain `%` and `//`; this model exists only
to say which branch of div_2by1 an input reaches, so that a test can state
(and tests/test_div32_model_cpu.py can prove from the oracle alone) that its
inputs run

    first:   if (rr > q0)  { --q1; rr += d; }
    second:  if (rr >= d)  { ++q1; rr -= d; }

both ways.  Each function returns its result(s) and the list of its
div_2by1 steps, one `Step` per call in program order.
"""
import collections
import contextlib

import numpy as np

import oracle as O

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1

Div32 = collections.namedtuple("Div32", "n sh dn v")

# first:   the first correction was taken
# second:  the second correction was taken
# exposed: the first correction was NOT taken and rr + d wraps past 2^32, so a
#          copy that applied the first correction unconditionally would not be
#          put right by the second (for rr + d < 2^32 the second undoes it).
Step = collections.namedtuple("Step", "first second exposed")


def make_div32(n):
    assert 0 < n <= M32
    sh = 32 - n.bit_length()
    dn = n << sh
    return Div32(n, sh, dn, M64 // dn - (1 << 32))


def div_2by1(u1, u0, d, v):
    """(u1:u0) / d for u1 < d, d normalised: (quotient word, remainder, Step)."""
    assert u1 < d and d >> 31 == 1
    q = (v * u1 + ((((u1 + 1) & M32) << 32) | u0)) & M64
    q1, q0 = q >> 32, q & M32
    rr = (u0 - q1 * d) & M32
    first = rr > q0
    exposed = (not first) and rr + d > M32
    if first:
        q1 = (q1 - 1) & M32
        rr = (rr + d) & M32
    second = rr >= d
    if second:
        q1 = (q1 + 1) & M32
        rr -= d
    return q1, rr, Step(first, second, exposed)


def divmod128(w, d):
    """w: four little-endian 32-bit words.  (remainder mod N, the low three
    quotient words [q0, q1, q2], steps)."""
    steps, q = [], [0, 0, 0]
    if d.sh == 0:
        r = w[3] - d.dn if w[3] >= d.dn else w[3]
        for i in (2, 1, 0):
            q[i], r, s = div_2by1(r, w[i], d.dn, d.v)
            steps.append(s)
        return r, q, steps
    sh = d.sh
    u = [(w[0] << sh) & M32] + [((w[i] << sh) | (w[i - 1] >> (32 - sh))) & M32 for i in (1, 2, 3)]
    r = w[3] >> (32 - sh)
    _, r, s = div_2by1(r, u[3], d.dn, d.v)
    steps.append(s)
    for i in (2, 1, 0):
        q[i], r, s = div_2by1(r, u[i], d.dn, d.v)
        steps.append(s)
    return r >> sh, q, steps


def mod32(x, d):
    sh = d.sh
    _, r, s = div_2by1(x >> (32 - sh) if sh else 0, (x << sh) & M32, d.dn, d.v)
    return r >> sh, [s]


def mul_mod(a, y, d):
    """(a * y) mod N for a < N and any 32-bit y."""
    assert a < d.n and y <= M32
    p = (a * y) << d.sh
    _, r, s = div_2by1(p >> 32, p & M32, d.dn, d.v)
    return r >> d.sh, [s]


def mod64(x, d):
    sh = d.sh
    hi, lo = x >> 32, x & M32
    r = hi >> (32 - sh) if sh else 0
    _, r, s1 = div_2by1(r, ((hi << sh) | (lo >> (32 - sh) if sh else 0)) & M32, d.dn, d.v)
    _, r, s2 = div_2by1(r, (lo << sh) & M32, d.dn, d.v)
    return r >> sh, [s1, s2]


def words(block):
    return [(block >> (32 * i)) & M32 for i in range(4)]


def sample(block0, next_words, mods):
    """The sampling of a tuple of IntModN<uint32_t, N_e> from the hashed
    blocks: r = block0; value_e = r mod N_e; r = (r / N_e) << 32 | next word.
    Returns (values, steps per leaf position)."""
    w, out, steps = words(block0), [], []
    for e, n in enumerate(mods):
        r, q, s = divmod128(w, make_div32(n))
        out.append(r)
        steps.append(s)
        if e + 1 < len(mods):
            w = [next_words[e], q[0], q[1], q[2]]
    return out, steps


def sample_reference(block0, next_words, mods):
    """The same rule with `%` and `//` on Python integers."""
    r, out = block0, []
    for e, n in enumerate(mods):
        out.append(r % n)
        if e + 1 < len(mods):
            r = (((r // n) << 32) | next_words[e]) & M128
    return out


class Census:
    """Branch counts over div_2by1 steps."""

    def __init__(self, steps=()):
        self.steps = self.first = self.skipped = self.second = self.exposed = 0
        self.add(steps)

    def add(self, steps):
        for s in steps:
            self.steps += 1
            self.first += s.first
            self.skipped += not s.first
            self.second += s.second
            self.exposed += s.exposed
        return self

    def merge(self, other):
        for k in ("steps", "first", "skipped", "second", "exposed"):
            setattr(self, k, getattr(self, k) + getattr(other, k))
        return self

    def both_ways(self):
        return self.first > 0 and self.skipped > 0

    def __repr__(self):
        return (f"Census(steps={self.steps}, first={self.first}, skipped={self.skipped}, "
                f"second={self.second}, exposed={self.exposed})")


# ---- the census of a whole test case, from the oracle's hashed value blocks ----------------
def value_blocks(seeds):
    """Hashes of `seed` and `seed + 1` under the value key, as Python integers:
    what every Mod32 leaf samples from."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1, 2)
    ints = O.ints_from_blocks(seeds)
    h0 = O.ints_from_blocks(O.aes_hash(O.PRG_KEY_VALUE, seeds))
    h1 = O.ints_from_blocks(O.aes_hash(O.PRG_KEY_VALUE, O.blocks_from_ints(
        [(s + 1) & M128 for s in ints])))
    return h0, h1


def sampling_census(seeds, mods, check=True):
    """Per leaf position e, the Census of divmod128 over the value blocks of
    `seeds` (expanded tree leaves, uint64 [n][2]).  With `check`, the model's
    values are compared with `%` and `//` on the way."""
    h0, h1 = value_blocks(seeds)
    out = [Census() for _ in mods]
    for a, b in zip(h0, h1):
        nw = words(b) + [0]
        vals, steps = sample(a, nw, mods)
        if check:
            assert vals == sample_reference(a, nw, mods)
        for c, s in zip(out, steps):
            c.add(s)
    return out


@contextlib.contextmanager
def recorded_value_seeds():
    """Collects the expanded seeds that the oracle's EvaluateUntil hashes into
    values (every call of O.hash_correct inside the block)."""
    seen, orig = [], O.hash_correct

    def record(vt, seeds, *args, **kwargs):
        seen.append(np.array(seeds, dtype=np.uint64).reshape(-1, 2))
        return orig(vt, seeds, *args, **kwargs)

    O.hash_correct = record
    try:
        yield seen
    finally:
        O.hash_correct = orig


def key_census(key, n, mods):
    """Census of one key's full domain of 2^n leaves (as _model_rows of
    test_full_domain_sketch_gpu.py walks it)."""
    cs, cl, cr = O._cw_arrays(key, 0, n)
    seeds, _ = O.expand_seeds(O.blocks_from_ints([key["seed"]]),
                              np.array([key["party"]], np.uint8), cs, cl, cr)
    return sampling_census(seeds, mods)


def merged(per_key):
    """Sum of per-position census lists."""
    out = [Census() for _ in per_key[0]]
    for cs in per_key:
        for a, b in zip(out, cs):
            a.merge(b)
    return out
