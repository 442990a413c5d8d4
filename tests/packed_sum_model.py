"""NumPy model of the packed full-domain sum's word arithmetic
(dpf_expand_sum.hip): word_add, the element-wise sum of two 64-bit words of 64 /
bits packed elements in which no carry crosses an element's top, and
reduce_lanes, the halving butterfly over the 64 lanes, with it."""
import numpy as np

DTYPE = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}
M64 = (1 << 64) - 1


def top_bits(bits):
    """H: the top bit of every element of a word."""
    return sum(1 << (e * bits + bits - 1) for e in range(64 // bits))


def word_add(a, b, bits):
    """word_add<bits> on uint64 arrays: 64 bits one add, 32 bits two 32-bit
    adds, below that the top bits added apart from the rest."""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    if bits == 64:
        return a + b
    if bits == 32:
        m = np.uint64(0xFFFFFFFF)
        s = np.uint64(32)
        return (((a >> s) + (b >> s)) & m) << s | ((a & m) + (b & m)) & m
    h = np.uint64(top_bits(bits))
    return ((a & ~h) + (b & ~h)) ^ ((a ^ b) & h)


def element_add(a, b, bits):
    """The definition: the words' elements added mod 2^bits."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    return (a.view(DTYPE[bits]) + b.view(DTYPE[bits])).view(np.uint64).reshape(a.shape)


def _shfl_xor(x, off):
    return x[np.arange(64) ^ off]


def butterfly(v, bits, xor):
    """reduce_lanes on v[lane][value] (NV = 2^H values per lane): H halving
    steps at offsets 32, 16, ..., in which a lane keeps the upper half of its
    values where its lane bit is set, sends the other half to its partner and
    adds what it gets; then the last value is summed over the remaining
    offsets.  Returns the word every lane ends with."""
    def op(x, y):
        return x ^ y if xor else word_add(x, y, bits)
    lanes = np.arange(64)
    v = np.array(v, dtype=np.uint64)
    nv, off = v.shape[1], 32
    while nv > 1:
        half = nv // 2
        up = ((lanes & off) != 0)[:, None]
        send = np.where(up, v[:, :half], v[:, half:nv])
        keep = np.where(up, v[:, half:nv], v[:, :half])
        v = op(keep, _shfl_xor(send, off))
        nv, off = half, off // 2
    r = v[:, 0]
    while off > 0:
        r = op(r, _shfl_xor(r, off))
        off //= 2
    return r
