"""The chunked work loop (take_chunk, dpf_device.h) of the DCF, MIC, point,
batch and key generation kernels on an MI355X.

Every AES-bound launcher hands its waves 64-item chunks from a per-workgroup
counter once the launch holds 4 chunks per wave of the chip
(chunked_shape, dpf_runtime.h): T = 4 * CUs * 1024 items, 2^20 on 256 CUs.  Below T
the same kernels run a grid-stride loop, and that is all the rest of the suite
reaches for these launchers.  Each case here is the smallest shape just above
T, with a chunk count that is no multiple of the grid, so that the last
workgroup with work owns fewer chunks than the others, at least one trailing
workgroup owns none and (where the shape allows) the last chunk is cut off by
the item count.

Every case runs the same device inputs twice, with default hooks and with the
launcher's DPF_*_DYNAMIC=0 hook; dpf_hip_last_dynamic_chunks tells which loop
ran (> 0 chunked, 0 grid stride).  The two output buffers are prefilled with
different bytes (an element neither run writes then differs between them) and
end in a 4 KiB guard that must stay untouched; the outputs must be equal byte
for byte, and the default run's rows at item 0, the last item, both sides of
two workgroup-range boundaries (b * per_wg * 64, per_wg from the diagnostic),
the last owning workgroup's short range and the cut-off chunk must equal the
references (oracle.py, mic_model.py).  All comparisons are bit-exact.

Key generation (keygen_kernel, DPF_KEYGEN_DYNAMIC) is the last section.  Its
item is a lane, two per key pair, and it writes several arrays per call: its
cases carve them out of one arena with an untouched gap after each
(keygen_common.KeygenArena) and compare every array of both schedules with the
host generator's batch, the boundary key pairs with the oracle's keys, and
evaluate every key pair at and next to its alpha.
"""
import numpy as np
import pytest

import mic_model as MM
import oracle as O
import ref_grids as G
from keygen_common import (assert_arrays_equal, batch_arrays, boundary_key_pairs, gen_into_arena,
                           oracle_arrays, rows_of, seed_ints)
from test_dcf_cpu import make as make_dcf
from test_host_api_cpu import leaves_value
from test_key_batch_cpu import make as make_dpf
from test_kernels_gpu import GENERIC_TYPES, _desc, _rand_blocks, _rand_value
from test_key_batch_gpu import _dev_points, _rand_u128, _setup
from test_mic_cpu import gate

pytestmark = pytest.mark.gpu

GUARD = 4096
KEYS3 = (O.PRG_KEY_LEFT, O.PRG_KEY_RIGHT, O.PRG_KEY_VALUE)


@pytest.fixture(scope="module")
def H():
    import torch
    from distributed_point_functions_amd import hip_abi
    hip_abi.load(require_gpu=True)
    assert torch.cuda.is_available()
    return hip_abi


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _threshold():
    """Items from which a launch of 1024-thread workgroups, one per CU, takes
    its work in chunks: 4 chunks of 64 per wave."""
    return 4 * _cus() * 1024


def _two_schedules(H, monkeypatch, hook, nbytes, launch):
    """launch(out) into two guarded buffers: default hooks (prefilled 0xAB, must
    report chunks > 0) and `hook`=0 (0x54, must report 0).  Returns the default
    run's bytes and its chunks per workgroup once both runs agree."""
    import torch
    got, per_wg = [], 0
    for fill, off in ((0xAB, False), (0x54, True)):
        if off:
            monkeypatch.setenv(hook, "0")
        else:
            monkeypatch.delenv(hook, raising=False)
        buf = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
        launch(buf[:nbytes])
        torch.cuda.synchronize()
        chunks = H.last_dynamic_chunks()
        if off:
            assert chunks == 0, (hook, chunks)
        else:
            assert chunks > 0, (hook, chunks)
            per_wg = chunks
        host = buf.cpu().numpy()
        assert bool((host[nbytes:] == fill).all()), f"guard tail written ({hook} off={off})"
        got.append(host[:nbytes])
    monkeypatch.delenv(hook)
    np.testing.assert_array_equal(got[0], got[1])
    return got[0], per_wg


def _boundary_items(n_items, per_wg, empty_tail=True):
    """Items where a wrong chunk-to-item mapping shows: item 0 and the last,
    the 64 on each side of two workgroup-range boundaries, and the whole range
    of the last workgroup that owns chunks (fewer than per_wg, the last of them
    cut off where n_items is no multiple of 64).  The grid is one workgroup
    per CU at these sizes, so a workgroup past `owners` owns nothing."""
    chunks = -(-n_items // 64)
    owners = -(-chunks // per_wg)
    assert per_wg == -(-chunks // _cus())
    assert owners < _cus() or not empty_tail, "no trailing workgroup without chunks"
    assert chunks % per_wg, "the last owning workgroup has a full share"
    span = per_wg * 64
    items = {0, n_items - 1}
    for b in (1, owners // 2):
        items.update(range(b * span - 64, b * span + 64))
    items.update(range((owners - 1) * span, n_items))
    return sorted(items)


# --------------------------------------------------------------------------
# The rule itself
# --------------------------------------------------------------------------

def test_threshold_edge(H):
    """dpf_hip_hash one chunk below T runs the grid-stride loop, at T the
    chunked one; both equal the oracle on sampled rows (outputs prefilled, so
    a row left unwritten cannot hold an earlier launch's value)."""
    import torch
    T = _threshold()
    rng = np.random.default_rng(1)
    x = _rand_blocks(rng, T)
    d = H.to_device_blocks(x)
    rows = np.unique(np.concatenate([[0, T - 65, T - 1], rng.integers(0, T, size=256)]))
    out = torch.full_like(d, 0x5454545454545454)
    below = H.blocks_to_numpy(H.hash_blocks(d[:T - 64], O.PRG_KEY_LEFT, out=out[:T - 64]))
    assert H.last_dynamic_chunks() == 0
    out.fill_(0x2B2B2B2B2B2B2B2B)
    at = H.blocks_to_numpy(H.hash_blocks(d, O.PRG_KEY_LEFT, out=out))
    assert H.last_dynamic_chunks() == T // 64 // _cus()
    want = O.aes_hash(O.PRG_KEY_LEFT, x[rows])
    np.testing.assert_array_equal(at[rows], want)
    np.testing.assert_array_equal(below[rows[rows < T - 64]], want[rows < T - 64])


# --------------------------------------------------------------------------
# DCF
# --------------------------------------------------------------------------

def dcf_rows(P, vt, okey, xs):
    """oracle.dcf_evaluate of one key at every x of xs, one EvaluateAt per
    level: the sum over levels i with bit n-1-i of x clear of
    EvaluateAt(key, i, x >> (n - i)) (n < 128).  Packed (len(xs), size)."""
    n = len(P.log_domain)
    assert n < 128
    acc = np.zeros((len(xs), O.packed_size(vt)), np.uint8)
    for i in range(n):
        e = O.evaluate_at(P, okey, i, [x >> (n - i) for x in xs]).copy()
        skip = np.array([(x >> (n - 1 - i)) & 1 for x in xs], bool)
        e[skip] = 0
        acc = O.add_packed(vt, acc, e)
    return acc


_KEYS = {}     # key batches shared by the cases of this module


def _dcf_keys(vt, n, nk):
    """nk party-mixed keys (key k: party k % 2) of the log-domain-n DCF, on
    the device, as test_dcf_gpu._batch_case makes them."""
    if ("dcf", repr(vt), n, nk) in _KEYS:
        return _KEYS["dcf", repr(vt), n, nk]
    dcf = make_dcf(vt, n)
    rng = np.random.default_rng(nk + len(repr(vt)))
    beta = [int(b) for b in rng.integers(1, 100, size=len(O.leaves(vt)))]
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=nk)]
    keys = [dcf.generate_keys(a, leaves_value(vt, beta), seed_0=2 * k + 1, seed_1=2 * k + 2)[k % 2]
            for k, a in enumerate(alphas)]
    _KEYS["dcf", repr(vt), n, nk] = dcf, beta, alphas, dcf.upload_key_batch(dcf.make_key_batch(keys))
    return _KEYS["dcf", repr(vt), n, nk]


def _dcf_case(H, monkeypatch, vt, nk, ppk, shared, general=False, n=16):
    """Both schedules of one DCF launch; whole rows of the keys that sit on the
    boundary items against the oracle.  Returns the default run's bytes."""
    import torch
    dcf, beta, alphas, dev = _dcf_keys(vt, n, nk)
    P = O.dcf_params(n, vt)
    rng = np.random.default_rng(ppk + shared)
    blocks = np.zeros((ppk if shared else nk * ppk, 2), np.uint64)
    blocks[:, 0] = rng.integers(0, 1 << n, size=len(blocks), dtype=np.uint64)
    if not shared:          # both comparison outcomes next to each key's alpha
        blocks[0::ppk, 0] = alphas
        blocks[1::ppk, 0] = np.maximum(np.array(alphas) - 1, 0)
    pts = blocks[:, 0].tolist()
    dpts = torch.from_numpy(blocks.view(np.int64)).cuda()
    size = dcf.packed_size()
    n_items = nk * ppk
    assert n_items >= _threshold()
    if general:
        monkeypatch.setenv("DPF_DCF_GENERAL", "1")

    def launch(out):
        assert dcf.evaluate_batch_to_device(dev, dpts, ppk, out, shared_points=shared) == n_items

    got, per_wg = _two_schedules(H, monkeypatch, "DPF_DCF_DYNAMIC", n_items * size, launch)
    got = got.reshape(nk, ppk, size)
    for k in sorted({u // ppk for u in _boundary_items(n_items, per_wg)}):
        okey = O.dcf_generate_keys(P, alphas[k], beta, 2 * k + 1, 2 * k + 2)[k % 2]
        xs = pts if shared else pts[k * ppk:(k + 1) * ppk]
        np.testing.assert_array_equal(got[k], dcf_rows(P, vt, okey, xs), err_msg=f"key {k}")
    return got


def test_dcf_rows_helper_equals_dcf_evaluate():
    """The per-level helper is oracle.dcf_evaluate, point by point."""
    vt = ("tuple", [("int", 16), ("intmodn", 128, G.M80)])
    P = O.dcf_params(7, vt)
    okey = O.dcf_generate_keys(P, 77, [5, 9], 3, 4)[1]
    xs = list(range(0, 128, 3)) + [76, 77, 78, 127]
    want = np.concatenate([O.dcf_evaluate(P, okey, x) for x in xs])
    np.testing.assert_array_equal(dcf_rows(P, vt, okey, xs), want)


@pytest.mark.parametrize("vt", [("int", 8), ("int", 64), ("int", 128), ("xor", 32)], ids=str)
def test_dcf_fast_kernel_chunked(H, vt, monkeypatch):
    """dcf_fast_kernel<.., UNIFORM = false>: (4 CUs + 7) keys x 1021 points
    (1031 x 1021 = 1,052,651 items on 256 CUs, 43 in the last chunk)."""
    _dcf_case(H, monkeypatch, vt, 4 * _cus() + 7, 1021, False)


@pytest.mark.parametrize("vt", [("int", 64), ("int", 128)], ids=str)
@pytest.mark.parametrize("shared", [False, True], ids=["per-key", "shared"])
def test_dcf_uniform_keys_chunked(H, vt, shared, monkeypatch):
    """(4 CUs + 3) keys x 1024 points: a wave's 64 items share one key, read
    through readfirstlane (dcf_fast_kernel<.., UNIFORM = true>), with per-key
    and with shared points; the general kernel (dcf_eval_kernel<.., true>,
    DPF_DCF_GENERAL=1) runs the same launch chunked and gives the same bytes."""
    nk = 4 * _cus() + 3
    fast = _dcf_case(H, monkeypatch, vt, nk, 1024, shared)
    general = _dcf_case(H, monkeypatch, vt, nk, 1024, shared, general=True)
    np.testing.assert_array_equal(fast, general)


def test_dcf_generic_kernel_chunked(H, monkeypatch):
    """A tuple value type takes dcf_eval_kernel<8, false> (GenericLeaf).  Log
    domain 10: the most at which one sample of the 80-bit modulus still meets
    a DCF level's security parameter (40 + its log domain <= 50 bits)."""
    vt = ("tuple", [("int", 16), ("intmodn", 128, G.M80)])
    _dcf_case(H, monkeypatch, vt, 4 * _cus() + 3, 1024, False, n=10)


# --------------------------------------------------------------------------
# Multiple interval containment
# --------------------------------------------------------------------------

def _dcf_cache(n, okey, points):
    """mic_model.evaluate's cache {point: DCF value}, filled level by level."""
    pts = sorted(set(points))
    rows = dcf_rows(MM.params(n), MM.VT, okey, pts)
    return dict(zip(pts, MM.ints_of(rows)))


class MicCase:
    """`gates` gates over one set of intervals: `pairs` distinct key pairs
    cycled over the gates (gate i holds pair i % pairs), a distinct masked
    input per gate."""

    def __init__(self, n, intervals, gates, seed, pairs=32):
        self.n, self.intervals, self.N, self.gates = n, intervals, 1 << n, gates
        self.g = gate(n, intervals)
        rng = np.random.default_rng(seed)
        m, N = len(intervals), self.N
        pairs = min(pairs, gates)
        self.r_in = [_big(rng, N) for _ in range(pairs)]
        self.r_out = [[_big(rng, N) for _ in range(m)] for _ in range(pairs)]
        self.z_0 = [[_big(rng, N) for _ in range(m)] for _ in range(pairs)]
        self.pairs = [self.g.gen(self.r_in[p], self.r_out[p], 2 * p + 1, 2 * p + 2, self.z_0[p])
                      for p in range(pairs)]
        edges = [v % N for p, q in intervals for v in (p, q, p - 1, q + 1)]
        self.x = [edges[int(rng.integers(0, len(edges)))] if i % 3 else _big(rng, N)
                  for i in range(gates)]
        self.masked = [(x + self.r_in[i % pairs]) % N for i, x in enumerate(self.x)]
        self.dev = {}

    def keys(self, flip):
        """Party (i + flip) % 2 of gate i."""
        np_ = len(self.pairs)
        return [self.pairs[i % np_][(i + flip) % 2] for i in range(self.gates)]

    def model_row(self, i, party):
        p = i % len(self.pairs)
        mk = MM.gen(self.n, self.intervals, self.r_in[p], self.r_out[p], 2 * p + 1, 2 * p + 2,
                    self.z_0[p])[party]
        N, x = self.N, self.masked[i]
        pts = [(x + N - 1 - b) % N for lo, hi in self.intervals for b in (lo, (hi + 1) % N)]
        return MM.evaluate(self.n, self.intervals, mk, x, _dcf_cache(self.n, mk["dcf"], pts))

    def run(self, flip, out):
        import torch
        if flip not in self.dev:
            self.dev[flip] = self.g.upload_key_batch(self.g.make_key_batch(self.keys(flip)))
        dx = torch.from_numpy(MM.u128_rows(self.masked).view(np.int64)).cuda()
        m = len(self.intervals)
        assert self.g.eval_batch_to_device(self.dev[flip], dx, out) == self.gates * m


def _big(rng, N):
    return int.from_bytes(rng.bytes(16), "little") % N


def _mic_chunked(H, monkeypatch, intervals, offsets, gates, seed):
    n = 12
    c = MicCase(n, intervals, gates, seed)
    m, U = len(intervals), c.g.num_unique_offsets()
    assert U == offsets
    walks = gates * U
    assert walks >= _threshold()
    shares = []
    for flip in (0, 1):
        got, per_wg = _two_schedules(H, monkeypatch, "DPF_DCF_DYNAMIC", gates * m * 16,
                                     lambda out: c.run(flip, out))
        v = got.view(np.uint64).reshape(gates, m, 2)
        assert not v[:, :, 1].any()
        shares.append(v[:, :, 0])
        # Walk item u belongs to gate u / |U|: the gates on the boundary items,
        # thinned to 24 (first and last kept).
        bg = sorted({u // U for u in _boundary_items(walks, per_wg)})
        if len(bg) > 24:
            bg = sorted({bg[round(j * (len(bg) - 1) / 23)] for j in range(24)})
        for i in bg:
            assert [int(s) for s in shares[flip][i]] == c.model_row(i, (i + flip) % 2), f"gate {i}"
    # Every gate by two-party reconstruction.
    mask = np.uint64(c.N - 1)
    r_out = np.array(c.r_out, np.uint64)[np.arange(gates) % len(c.pairs)]
    rec = (shares[0] + shares[1] - r_out) & mask
    x = np.array(c.x, np.uint64)[:, None]
    lo = np.array([p for p, _ in intervals], np.uint64)[None, :]
    hi = np.array([q for _, q in intervals], np.uint64)[None, :]
    np.testing.assert_array_equal(rec, ((lo <= x) & (x <= hi)).astype(np.uint64))


def test_mic_walk_kernel_chunked(H, monkeypatch):
    """mic_walk_kernel<false>: 16 non-adjacent intervals, |U| = 32, T / 32 + 3
    gates (32,771 on 256 CUs: 1,048,672 walks, 32 in the last chunk)."""
    intervals = MM.disjoint(12, 16, np.random.default_rng(16))
    _mic_chunked(H, monkeypatch, intervals, 32, _threshold() // 32 + 3, seed=32)


def test_mic_walk_kernel_uniform_chunked(H, monkeypatch):
    """mic_walk_kernel<true>: a 64-way partition, |U| = 64, every wave walks
    one gate's key through readfirstlane; T / 64 + 16 gates (16,400)."""
    _mic_chunked(H, monkeypatch, MM.partition(12, 64), 64, _threshold() // 64 + 16, seed=64)


def test_mic_walk_kernel_uniform_n127(H):
    """The wave-uniform form at the largest group: 2 gates x a 64-way
    partition of Z_{2^127}, both parties equal to the model on every share.
    128 walks: the grid-stride loop."""
    import torch
    n = 127
    c = MicCase(n, MM.partition(n, 64), 2, seed=127)
    assert c.g.num_unique_offsets() == 64
    m = 64
    shares = []
    for flip in (0, 1):
        out = torch.full((2 * m * 16 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        c.run(flip, out[:2 * m * 16])
        torch.cuda.synchronize()
        assert H.last_dynamic_chunks() == 0
        host = out.cpu().numpy()
        assert bool((host[2 * m * 16:] == 0xAB).all())
        flat = MM.ints_of(host[:2 * m * 16])
        shares.append([flat[:m], flat[m:]])
        for i in range(2):
            assert shares[flip][i] == c.model_row(i, (i + flip) % 2), f"gate {i} flip {flip}"
    for i in range(2):
        assert MM.reconstruct(n, shares[0][i], shares[1][i], c.r_out[i]) == \
            MM.contains(c.intervals, c.x[i])


# --------------------------------------------------------------------------
# Point evaluation, two chains per lane (raw ABI, random key material)
# --------------------------------------------------------------------------

def _points_case(H, monkeypatch, vt, num_keys, ppk, levels, from_partials=False, sec=48.0):
    """test_kernels_gpu._points_case at a chunked size: both schedules, every
    row against the oracle."""
    import torch
    rng = np.random.default_rng(ppk + num_keys)
    b = (O.bits_needed(vt, sec) + 127) // 128
    E = O.elements_per_block(vt)
    n = num_keys * ppk
    assert num_keys * ((ppk + 1) // 2) >= _threshold()      # an item is a pair of points
    key_seed = _rand_blocks(rng, num_keys)
    party = rng.integers(0, 2, size=num_keys, dtype=np.uint8)
    cws = _rand_blocks(rng, num_keys * levels)
    cl = rng.integers(0, 2, size=num_keys * levels, dtype=np.uint8)
    cr = rng.integers(0, 2, size=num_keys * levels, dtype=np.uint8)
    assert levels < 64
    tree = np.zeros((n, 2), np.uint64)
    tree[:, 0] = rng.integers(0, 1 << levels, size=n, dtype=np.uint64)
    bi = rng.integers(0, E, size=n, dtype=np.int32)
    vcws = [[_rand_value(rng, vt) for _ in range(E)] for _ in range(num_keys)]
    seeds_in = _rand_blocks(rng, n) if from_partials else None
    ctrl_in = rng.integers(0, 2, size=n, dtype=np.uint8) if from_partials else None
    esz = O.packed_size(vt)
    dev = dict(key_seed=H.to_device_blocks(key_seed), party=H.to_device_u8(party),
               tree=H.to_device_blocks(tree), bi=torch.from_numpy(bi).cuda(),
               cws=H.to_device_blocks(cws), cl=H.to_device_u8(cl), cr=H.to_device_u8(cr),
               vcw=H.to_device_blocks(O._leaf_array([e for v in vcws for e in v])),
               seeds_in=H.to_device_blocks(seeds_in) if from_partials else None,
               ctrl_in=H.to_device_u8(ctrl_in) if from_partials else None)

    def launch(out):
        H.eval_points(n, ppk, levels, dev["key_seed"], dev["party"], dev["tree"], dev["bi"],
                      dev["cws"], dev["cl"], dev["cr"], KEYS3, _desc(H, vt, b), dev["vcw"],
                      seeds_in=dev["seeds_in"], ctrl_in=dev["ctrl_in"], out=out)
        assert H.last_points_kernel() == "points/ilp2"

    got, _ = _two_schedules(H, monkeypatch, "DPF_POINTS_DYNAMIC", n * esz, launch)
    got = got.reshape(n, esz)
    for k in range(num_keys):
        sl = slice(k * ppk, (k + 1) * ppk)
        lv = slice(k * levels, (k + 1) * levels)
        if from_partials:
            s0, c0 = seeds_in[sl], ctrl_in[sl]
        else:
            s0 = np.repeat(key_seed[k:k + 1], ppk, axis=0)
            c0 = np.full(ppk, party[k], np.uint8)
        s, c = O.evaluate_seeds(s0, c0, tree[sl], cws[lv], cl[lv], cr[lv])
        want = O.hash_select_correct(vt, s, c, b, bi[sl], vcws[k], int(party[k]))
        np.testing.assert_array_equal(got[sl], want, err_msg=f"key {k}")


def test_eval_points_kernel_chunked_one_key(H, monkeypatch):
    """eval_points_kernel, 1 key x (2 T + 77) points (2^21 + 77), 8 levels."""
    _points_case(H, monkeypatch, ("int", 64), 1, 2 * _threshold() + 77, 8)


def test_eval_points_kernel_chunked_from_partials(H, monkeypatch):
    """3 keys x 699,073 points from partial evaluations: items of different
    keys share chunks (ragged halves)."""
    ppk = 2 * (_threshold() // 3 + 12) - 1
    _points_case(H, monkeypatch, ("xor", 128), 3, ppk, 8, from_partials=True)


def test_eval_points_kernel_chunked_generic_leaf(H, monkeypatch):
    """GenericLeaf (Tuple<uint32, uint64>) in the chunked loop."""
    _points_case(H, monkeypatch, GENERIC_TYPES[0], 1, 2 * _threshold() + 77, 8)


# --------------------------------------------------------------------------
# Point evaluation, four chains per lane (product API)
# --------------------------------------------------------------------------

def _dpf_keys(levels, n_keys, seed):
    """test_key_batch_gpu._setup's party-mixed batch, on the device."""
    if ("dpf", repr(levels), n_keys) not in _KEYS:
        dpf, P, _, batch, oks, _, _, _ = _setup(levels, n_keys, seed=seed)
        _KEYS["dpf", repr(levels), n_keys] = dpf, P, dpf.upload_key_batch(batch), oks
    return _KEYS["dpf", repr(levels), n_keys]


@pytest.mark.parametrize("bits,tops", [(64, (None, "0")), (128, (None,))], ids=["u64", "u128"])
def test_eval_points4_kernel_chunked(H, bits, tops, monkeypatch):
    """eval_points4_kernel: (4 CUs + 76) keys x 4096 shared points (1100 x 1024
    items) on a 2^24 domain, per key and summed over keys, with the shared
    top walk and (uint64) with DPF_POINTS_SHARED_TOP=0.  All forms of one
    output agree byte for byte; the keys on the boundary items equal the
    oracle's EvaluateAt; the sum is the wrap-around sum of the per-key rows."""
    levels = [(24, ("int", bits), 0)]
    n_keys, npts = 4 * _cus() + 76, 4096
    quarter = npts // 4
    dpf, P, dev, oks = _dpf_keys(levels, n_keys, 24)
    pts = _rand_u128(np.random.default_rng(bits), npts, 24)
    dpts = _dev_points(pts)
    size = bits // 8
    assert n_keys * quarter >= _threshold()

    def per_key(out):
        assert dpf.evaluate_at_batch_to_device(dev, 0, dpts, npts, out,
                                               shared_points=True) == n_keys * npts
        assert H.last_points_kernel() == "points/ilp4"

    def summed(out):
        dpf.evaluate_at_batch_sum_to_device(dev, 0, dpts, out)
        assert H.last_points_kernel() == "points/ilp4"

    rows, sums, per_wg = [], [], 0
    for top in tops:
        if top is None:
            monkeypatch.delenv("DPF_POINTS_SHARED_TOP", raising=False)
        else:
            monkeypatch.setenv("DPF_POINTS_SHARED_TOP", top)
        got, per_wg = _two_schedules(H, monkeypatch, "DPF_POINTS_DYNAMIC",
                                     n_keys * npts * size, per_key)
        rows.append(got)
        got, sum_per_wg = _two_schedules(H, monkeypatch, "DPF_POINTS_DYNAMIC", npts * size, summed)
        sums.append(got)
        assert sum_per_wg == per_wg        # one key per item row in both forms
    for other in rows[1:]:
        np.testing.assert_array_equal(rows[0], other)
    for other in sums[1:]:
        np.testing.assert_array_equal(sums[0], other)
    got = rows[0].reshape(n_keys, npts, size)
    # Item u is key u / quarter (its four points j, j + quarter, ...).  On 256
    # CUs the 17,600 chunks are 69 per workgroup: all 256 own some, the last 5.
    bk = sorted({u // quarter
                 for u in _boundary_items(n_keys * quarter, per_wg, empty_tail=False)})
    if len(bk) > 8:
        bk = sorted({bk[round(j * (len(bk) - 1) / 7)] for j in range(8)})
    for k in bk:
        np.testing.assert_array_equal(got[k], O.evaluate_at(P, oks[k], 0, pts), err_msg=f"key {k}")
    words = got.view(np.uint64).reshape(n_keys, npts * (size // 8))
    if bits == 64:
        total = words.sum(axis=0, dtype=np.uint64)
    else:
        # Low words summed in 32-bit halves: the carries into the high word.
        lo, hi = words[:, 0::2], words[:, 1::2]
        s32 = np.uint64(32)
        low_half = (lo & np.uint64(0xFFFFFFFF)).sum(axis=0, dtype=np.uint64)
        high_half = (lo >> s32).sum(axis=0, dtype=np.uint64) + (low_half >> s32)
        total = np.empty(npts * 2, np.uint64)
        total[0::2] = lo.sum(axis=0, dtype=np.uint64)
        total[1::2] = hi.sum(axis=0, dtype=np.uint64) + (high_half >> s32)
    np.testing.assert_array_equal(sums[0].view(np.uint64), total)


# --------------------------------------------------------------------------
# Batched EvaluateUntil
# --------------------------------------------------------------------------

BATCH_LEVELS = [(10, ("int", 64), 0), (12, ("int", 64), 0)]


@pytest.mark.parametrize("no_cache", [False, True], ids=["cached", "walked"])
@pytest.mark.parametrize("sum_mode", [False, True], ids=["per-key", "sum"])
def test_batch_level_kernel_chunked(H, no_cache, sum_mode, monkeypatch):
    """batch_level_kernel: level 0, then level 1 at 1000 of its 1024 prefixes,
    start seeds from the expansion cache and (DPF_BATCH_NO_CACHE=1) walked from
    the roots, per key and summed over keys.

    Two uint64 share a block, so the 1000 prefixes are 500 tree nodes: 8 wave
    tasks per key, the last ragged (52 nodes).  The launch is chunked from
    4 x 16 x CUs tasks, one key per task row: 8 CUs + 6 keys (2054; with 1030
    keys the launch has 8240 tasks and runs the grid-stride loop on 256 CUs).
    DPF_BATCH_DYNAMIC=0 also regroups the keys (plan_key_chunks: 4 instead of
    16 tasks per wave slot): the bytes must not change."""
    import torch
    if no_cache:
        monkeypatch.setenv("DPF_BATCH_NO_CACHE", "1")
    prefixes = list(range(1000))
    starts = len({p >> 1 for p in prefixes})
    waves = -(-starts // 64)
    assert starts % 64
    n_keys = -(-_cus() * 64 // waves) + 6
    dpf, P, dev, oks = _dpf_keys(BATCH_LEVELS, n_keys, 1030)
    size = dpf.packed_size(1)
    n_out = dpf.output_elements(1, len(prefixes), 0)
    assert n_out == 4 * len(prefixes)
    rows = 1 if sum_mode else n_keys

    def launch(out):
        bctx = dpf.create_batch_evaluation_context(dev)
        first = torch.empty(rows * dpf.output_elements(0, 0, -1) * dpf.packed_size(0),
                            dtype=torch.uint8, device="cuda")
        dpf.evaluate_until_batch_to_device(0, [], bctx, first, sum_over_keys=sum_mode)
        assert dpf.evaluate_until_batch_to_device(1, prefixes, bctx, out,
                                                  sum_over_keys=sum_mode) == n_out
        assert H.last_batch_kernel() == "batch_level/fast"

    got, per_wg = _two_schedules(H, monkeypatch, "DPF_BATCH_DYNAMIC", rows * n_out * size, launch)
    got = got.reshape(rows, n_out, size)

    def oracle_row(k):
        ctx = O.create_context(P, oks[k])
        O.evaluate_until(P, 0, [], ctx)
        return O.evaluate_until(P, 1, prefixes, ctx)

    if sum_mode:
        # The per-key launch of the same keys and prefixes (checked against the
        # oracle in the per-key case) summed in numpy.
        monkeypatch.delenv("DPF_BATCH_DYNAMIC", raising=False)
        each = torch.empty(n_keys * n_out * size, dtype=torch.uint8, device="cuda")
        bctx = dpf.create_batch_evaluation_context(dev)
        first = torch.empty(n_keys * dpf.output_elements(0, 0, -1) * dpf.packed_size(0),
                            dtype=torch.uint8, device="cuda")
        dpf.evaluate_until_batch_to_device(0, [], bctx, first)
        dpf.evaluate_until_batch_to_device(1, prefixes, bctx, each)
        torch.cuda.synchronize()
        total = each.cpu().numpy().view(np.uint64).reshape(n_keys, n_out).sum(axis=0, dtype=np.uint64)
        np.testing.assert_array_equal(got.view(np.uint64).reshape(n_out), total)
        return
    # Wave task g is key g / waves (one key per task row on the default run).
    bk = sorted({g // waves for g in
                 (u // 64 for u in _boundary_items(n_keys * waves * 64, per_wg))})
    if len(bk) > 8:
        bk = sorted({bk[round(j * (len(bk) - 1) / 7)] for j in range(8)})
    for k in bk:
        np.testing.assert_array_equal(got[k], oracle_row(k), err_msg=f"key {k}")


# --------------------------------------------------------------------------
# Key generation
# --------------------------------------------------------------------------

def _keygen_count():
    """T / 2 + 113 key pairs: T + 226 lanes, the smallest count just above the
    threshold whose T / 64 + 4 chunks leave the last owning workgroup a short
    range (8 of per_wg = 65 chunks on 256 CUs, three workgroups without any)
    and whose last chunk is cut inside a wave (34 lanes, 17 key pairs).
    _boundary_items asserts the first two conditions for the chip it runs on:
    they hold from 69 CUs up (per_wg is 65 wherever 4 < CUs)."""
    K = _threshold() // 2 + 113
    assert -(-2 * K // 64) == _threshold() // 64 + 4 and 2 * K % 64 == 34
    return K


def _keygen_inputs(seed, K, top, fixed):
    """(K, 2) uint64 alphas below 2^top (`fixed` first, random after) and
    (2 K, 2) root seeds, [key][party]."""
    rng = np.random.default_rng(seed)
    alphas = np.zeros((K, 2), np.uint64)
    alphas[:, 0] = rng.integers(0, 1 << top, size=K, dtype=np.uint64)
    alphas[:len(fixed), 0] = fixed
    seeds = rng.integers(0, 1 << 63, size=(2 * K, 2), dtype=np.uint64)
    return rng, alphas, seeds


def _beta_pool(rng, vt, K, first=()):
    """One beta leaf per key as a uint64 array and as Values: `first`, then
    random draws from a pool of 1024 random leaves (one Value object per pool
    entry; building K of them would take longer than the launch under test)."""
    bits = O.leaves(vt)[0][1]
    assert bits <= 64
    pool = rng.integers(0, 1 << (bits - 1), size=1024, dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=1024, dtype=np.uint64)
    pool[:len(first)] = np.array(first, np.uint64)
    pick = rng.integers(0, 1024, size=K)
    pick[:len(first)] = np.arange(len(first))
    values = [leaves_value(vt, [int(v)]) for v in pool]
    return pool[pick], [values[i] for i in pick]


def _keygen_two_schedules(H, monkeypatch, run):
    """run(fill) -> the arrays of one key generation call, under the default
    hooks (must report chunks > 0) and with DPF_KEYGEN_DYNAMIC=0 (must report
    0), prefilled with different bytes where the caller owns the buffers.
    Returns the default run's arrays and its chunks per workgroup once every
    array of the two runs is equal."""
    hook = "DPF_KEYGEN_DYNAMIC"
    got, per_wg = [], 0
    for fill, off in ((0xAB, False), (0x54, True)):
        if off:
            monkeypatch.setenv(hook, "0")
        else:
            monkeypatch.delenv(hook, raising=False)
        arrays, chunks = run(fill)
        if off:
            assert chunks == 0, (hook, chunks)
        else:
            assert chunks > 0, (hook, chunks)
            per_wg = chunks
        got.append(arrays)
    monkeypatch.delenv(hook)
    assert got[0].keys() == got[1].keys()
    assert_arrays_equal(got[0], got[1], "DPF_KEYGEN_DYNAMIC=0 against the default")
    return got[0], per_wg


def _abi_runner(H, P, K, d_alphas, d_seeds, d_beta, beta_mode):
    import torch

    def run(fill):
        arena = gen_into_arena(H, P, K, d_alphas, d_seeds, d_beta, beta_mode, fill)
        chunks = H.last_dynamic_chunks()
        torch.cuda.synchronize()
        return arena.arrays(), chunks     # asserts the gaps and the guard
    return run


def _shares(dev, evaluate, pts, ppk, size):
    """Both parties' packed outputs at `pts` (ppk per key) as (K * ppk, size)."""
    import torch
    outs = []
    d_pts = torch.from_numpy(np.ascontiguousarray(pts).view(np.int64)).cuda()
    for d in dev:
        out = torch.empty(len(pts) * size, dtype=torch.uint8, device="cuda")
        assert evaluate(d, d_pts, ppk, out) == len(pts)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    return outs


def _recombine(vt, a, b):
    kind, bits, _ = O.leaves(vt)[0]
    dt = {32: np.uint32, 64: np.uint64}[bits]
    return a.view(dt) ^ b.view(dt) if kind == O.LEAF_XOR else a.view(dt) + b.view(dt)


def _points(cols):
    """(K * len(cols), 2) uint64 points, key-major, from per-key columns."""
    pts = np.zeros((len(cols[0]), len(cols), 2), np.uint64)
    for j, c in enumerate(cols):
        pts[:, j, 0] = c
    return pts.reshape(-1, 2)


def _check_dpf_keys(dpf, levels, dev, alphas, betas):
    """Every key pair: shares of betas[h][k] at alpha's prefix of level h and
    of 0 at the prefix with its lowest bit flipped."""
    top = levels[-1][0]
    for h, (log, vt, _) in enumerate(levels):
        prefix = alphas[:, 0] >> np.uint64(top - log)
        outs = _shares(dev, lambda d, p, n, o: dpf.evaluate_at_batch_to_device(d, h, p, n, o),
                       _points([prefix, prefix ^ np.uint64(1)]), 2, dpf.packed_size(h))
        got = _recombine(vt, *outs).reshape(-1, 2)
        np.testing.assert_array_equal(got[:, 0], betas[h].astype(got.dtype), err_msg=f"level {h}")
        assert not got[:, 1].any(), f"level {h}"


def _oracle_rows(P, got, K, per_wg, okey, limit=48):
    """The boundary key pairs against the oracle's single-key generation.  The
    two cases that take longer than the other tests of this module (their host
    generator reads one Value per key) keep 24: the first and the last pair,
    the cut-off chunk, both sides of the two boundaries and two more."""
    ks = boundary_key_pairs(K, per_wg, limit)
    assert_arrays_equal(rows_of(got, ks, K), oracle_arrays(P, [okey(k) for k in ks]),
                        "boundary key pairs")


def test_keygen_kernel_chunked_shared_betas(H, monkeypatch):
    """beta_mode 0 through the C ABI, one uint32 level of log domain 7: L = 5,
    one run of four levels and a tail of one, and, L being odd, control bytes
    4-aligned for every second key only.  Beta all ones; alphas 0, all ones and
    random."""
    levels = [(7, ("int", 32), 0)]
    vt, beta = levels[0][1], (1 << 32) - 1
    P = O.OracleParams(levels)
    assert P.tree_levels_needed - 1 == 5
    K = _keygen_count()
    rng, alphas, seeds = _keygen_inputs(7, K, 7, [0, 127])
    values = [leaves_value(vt, [beta])]
    run = _abi_runner(H, P, K, H.to_device_blocks(alphas), H.to_device_blocks(seeds),
                      H.to_device_blocks(np.array([[beta, 0]], np.uint64)), 0)
    got, per_wg = _keygen_two_schedules(H, monkeypatch, run)
    dpf = make_dpf(levels)
    host = dpf.generate_key_batch(alphas, values, root_seeds=seeds)
    assert_arrays_equal(got, batch_arrays(host[0]), "host batch")
    _oracle_rows(P, got, K, per_wg,
                 lambda k: O.generate_keys(P, int(alphas[k, 0]), [[beta]], *seed_ints(seeds, k))[0])
    del host
    # The same call through the API: the same bytes, and the keys they hold.
    dev = dpf.generate_key_batch_to_device(alphas, values, root_seeds=seeds)
    assert H.last_dynamic_chunks() == per_wg
    assert_arrays_equal(got, batch_arrays(dpf.download_key_batch(dev[0])), "API")
    _check_dpf_keys(dpf, levels, dev, alphas, [np.full(K, beta, np.uint64)])


def test_keygen_kernel_chunked_per_key_betas(H, monkeypatch):
    """beta_mode 1 through generate_key_batch_to_device and download_key_batch:
    uint32 at log domain 5 under XorWrapper<uint64> at 9, tree levels [3, 8],
    L = 8, two full runs.  Betas 0 and all ones for the first two keys, random
    after.  A DeviceKeyBatch of this size generates, downloads and evaluates."""
    levels = [(5, ("int", 32), 0), (9, ("xor", 64), 0)]
    P = O.OracleParams(levels)
    assert list(P.hierarchy_to_tree) == [3, 8] and P.tree_levels_needed - 1 == 8
    K = _keygen_count()
    rng, alphas, seeds = _keygen_inputs(9, K, 9, [0, 511])
    betas, cols = [], []
    for _, vt, _ in levels:
        b, v = _beta_pool(rng, vt, K, first=[0, (1 << O.leaves(vt)[0][1]) - 1])
        betas.append(b)
        cols.append(v)
    values = [v for pair in zip(*cols) for v in pair]      # key-major
    dpf = make_dpf(levels)
    assert dpf.generates_keys_on_device()
    kept = {}

    def run(fill):
        dev = dpf.generate_key_batch_to_device(alphas, values, root_seeds=seeds)
        chunks = H.last_dynamic_chunks()
        kept.setdefault("dev", dev)                        # the default run's keys
        parties = [batch_arrays(dpf.download_key_batch(d)) for d in dev]
        return {f"{name}/{p}": a for p in (0, 1) for name, a in parties[p].items()}, chunks

    got, per_wg = _keygen_two_schedules(H, monkeypatch, run)
    host = dpf.generate_key_batch_with_betas(alphas, values, root_seeds=seeds)
    for p in (0, 1):
        mine = {name[:-2]: a for name, a in got.items() if name.endswith(f"/{p}")}
        assert_arrays_equal(mine, batch_arrays(host[p]), f"host batch, party {p}")
        assert set(mine) == set(batch_arrays(host[p]))     # seeds and party bytes too
        _oracle_rows(P, mine, K, per_wg,
                     lambda k: O.generate_keys(P, int(alphas[k, 0]),
                                               [[int(b[k])] for b in betas],
                                               *seed_ints(seeds, k))[p], limit=24)
    del host
    _check_dpf_keys(dpf, levels, kept["dev"], alphas, betas)


def test_keygen_kernel_chunked_dcf(H, monkeypatch):
    """beta_mode 2 through the C ABI: the uint64 DCF of log domain 8, H = 8,
    L = 7 with a tail of three, one beta per key, every alpha of [0, 256)
    among the keys.  Evaluated at alpha - 1, alpha and 255: beta below alpha,
    else 0."""
    n, vt = 8, ("int", 64)
    P = O.dcf_params(n, vt)
    assert len(P.log_domain) == 8 and P.tree_levels_needed - 1 == 7
    K = _keygen_count()
    rng, alphas, seeds = _keygen_inputs(8, K, n, np.arange(256))
    assert set(alphas[:, 0].tolist()) == set(range(256))
    beta, values = _beta_pool(rng, vt, K, first=[0, (1 << 64) - 1])
    d_beta = np.zeros((K, 2), np.uint64)
    d_beta[:, 0] = beta
    run = _abi_runner(H, P, K, H.to_device_blocks(alphas), H.to_device_blocks(seeds),
                      H.to_device_blocks(d_beta), 2)
    got, per_wg = _keygen_two_schedules(H, monkeypatch, run)
    dcf = make_dcf(vt, n)
    host = dcf.generate_key_batch(alphas, values, root_seeds=seeds)
    assert_arrays_equal(got, batch_arrays(host[0]), "host batch")
    _oracle_rows(P, got, K, per_wg,
                 lambda k: O.dcf_generate_keys(P, int(alphas[k, 0]), [int(beta[k])],
                                               *seed_ints(seeds, k))[0], limit=24)
    del host
    dev = dcf.generate_key_batch_to_device(alphas, values, root_seeds=seeds)
    assert H.last_dynamic_chunks() == per_wg
    assert_arrays_equal(got, batch_arrays(dcf.download_key_batch(dev[0])), "API")
    a = alphas[:, 0]
    cols = [(a - np.uint64(1)) & np.uint64(255), a, np.full(K, 255, np.uint64)]
    outs = _shares(dev, lambda d, p, m, o: dcf.evaluate_batch_to_device(d, p, m, o),
                   _points(cols), 3, dcf.packed_size())
    rec = _recombine(vt, *outs).reshape(K, 3)
    for j, x in enumerate(cols):
        np.testing.assert_array_equal(rec[:, j], np.where(x < a, beta, np.uint64(0)),
                                      err_msg=f"point {j}")
