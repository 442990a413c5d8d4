"""Batched key generation on an MI355X (dpf_hip_gen_key_batch through
generate_key_batch_to_device, the DCF's and the MIC gate's): every array of both
downloaded batches is byte-equal to the host batch from the same root seeds and
to the CPU oracle's keys, and -- independently of any host key generation -- the
device-generated keys evaluate to shares of beta at alpha and of 0 elsewhere."""
import numpy as np
import pytest

import mic_model as MM
import oracle as O
import ref_grids as G
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import mic as M
from keygen_common import (EDGE_LEVELS, KeygenArena, assert_arrays_equal,
                           assert_batch_equals_oracle, assert_batches_equal, batch_arrays,
                           seed_ints)
from test_dcf_cpu import make as make_dcf
from test_host_api_cpu import leaves_value
from test_key_batch_cpu import make, seeds_array

pytestmark = pytest.mark.gpu

MIXED = [(3, ("int", 8), 0), (10, ("int", 128), 0), (20, ("xor", 64), 0)]
# (levels, key counts): the depths L = 0, 1, 4, 5 and 127, then every leaf width.
CASES = [
    ([(2, ("int", 32), 0)], (1, 33, 513)),     # L = 0: the domain is one block
    ([(3, ("int", 32), 0)], (1, 33, 513)),     # L = 1
    ([(6, ("int", 32), 0)], (1, 33, 513)),     # L = 4: one full run of four levels
    ([(7, ("int", 32), 0)], (1, 33, 513)),     # L = 5: a run and its tail
    ([(128, ("int", 64), 0)], (33,)),          # L = 127
    ([(9, ("int", 8), 0)], (33,)),             # 16 elements per block
    ([(8, ("int", 16), 0)], (33,)),
    ([(9, ("int", 64), 0)], (33,)),            # L = 8: two full runs
    ([(11, ("int", 128), 0)], (33,)),          # L = 11: tail of three
    ([(7, ("xor", 64), 0)], (33,)),            # L = 6: tail of two
    (MIXED, (33, 513)),
    # The level-table edges: the shift by 128 (alphas with bit 127 set and clear),
    # every width at an inner level with 4, 3, 2, 1 and 0 index bits, and value
    # corrections from consecutive tree levels.
    *[(levels, (33,)) for levels, _ in EDGE_LEVELS],
]


def _alphas(rng, n, top):
    mask = (1 << top) - 1
    fixed = [0, mask, ((1 << 127) | (1 << 70) | 5) & mask]
    rand = [int.from_bytes(rng.bytes(16), "little") & mask for _ in range(n)]
    return (fixed + rand)[:n] if n >= 3 else rand[:n]


def _beta_leaf(vt, k, rng):
    bits = O.leaves(vt)[0][1]
    if k == 0:
        return 0
    if k == 1:
        return (1 << bits) - 1
    return int.from_bytes(rng.bytes(16), "little") % (1 << bits)


def _dev_points(pts):
    import torch
    return torch.from_numpy(D.u128_array(pts).view(np.int64)).cuda()


def _ints(packed, size):
    return [int.from_bytes(bytes(r), "little") for r in packed.reshape(-1, size)]


def _evaluate(dpf, dev, h, pts, ppk, stream=None):
    import torch
    size = dpf.packed_size(h)
    out = torch.empty(dev.num_keys * ppk * size, dtype=torch.uint8, device="cuda")
    assert dpf.evaluate_at_batch_to_device(dev, h, _dev_points(pts), ppk, out,
                                           stream=stream) == dev.num_keys * ppk
    torch.cuda.synchronize()
    return _ints(out.cpu().numpy(), size)


def _check_point_function(dpf, levels, d0, d1, alphas, beta_of, only=None):
    """Shares sum to beta at alpha and to 0 at its neighbours, at every level
    (of `only`): the prefix with its lowest bit and with every bit flipped and,
    where the level's block holds several elements, the point of the prefix's
    own block whose index differs in the top bit (a level of log domain 0 has
    the one point 0)."""
    top = levels[-1][0]
    tree = dpf.hierarchy_to_tree()
    for h, (log, vt, _) in enumerate(levels):
        if only is not None and h not in only:
            continue
        kind, bits, _ = O.leaves(vt)[0]
        index_bits = log - tree[h]
        assert 0 <= index_bits and (1 << index_bits) <= 128 // bits
        flips = (0, 1 if log else 0, (1 << log) - 1, (1 << index_bits) >> 1)
        prefixes = [a >> (top - log) for a in alphas]
        pts = [p ^ d for p in prefixes for d in flips]
        y0, y1 = _evaluate(dpf, d0, h, pts, 4), _evaluate(dpf, d1, h, pts, 4)
        for k, p in enumerate(prefixes):
            for j in range(4):
                x = pts[4 * k + j]
                a, b = y0[4 * k + j], y1[4 * k + j]
                got = a ^ b if kind == O.LEAF_XOR else (a + b) % (1 << bits)
                assert got == (beta_of(k, h) if x == p else 0), (h, k, j)


@pytest.mark.parametrize("per_key", [False, True], ids=["shared", "per_key"])
@pytest.mark.parametrize("levels,counts", CASES, ids=str)
def test_device_batches_equal_host_and_oracle(levels, counts, per_key):
    dpf = make(levels)
    assert dpf.generates_keys_on_device()
    P = O.OracleParams(levels)
    H = len(levels)
    for n in counts:
        rng = np.random.default_rng(n + levels[-1][0])
        alphas = _alphas(rng, n, levels[-1][0])
        seeds = seeds_array(rng, n)
        rows = n if per_key else 1
        # Per key: 0 and all ones for the first two keys; shared: all ones.
        leaves = [[[_beta_leaf(vt, r if per_key else 1, rng)] for _, vt, _ in levels]
                  for r in range(rows)]
        values = [leaves_value(vt, leaves[r][h]) for r in range(rows)
                  for h, (_, vt, _) in enumerate(levels)]
        if per_key:
            host = dpf.generate_key_batch_with_betas(alphas, values, root_seeds=seeds)
        else:
            host = dpf.generate_key_batch(alphas, values, root_seeds=seeds)
        dev = dpf.generate_key_batch_to_device(alphas, values, root_seeds=seeds)
        got = [dpf.download_key_batch(d) for d in dev]
        beta_of = lambda k, h: leaves[k if per_key else 0][h][0]   # noqa: E731
        okeys = [O.generate_keys(P, alphas[k], leaves[k if per_key else 0], *seed_ints(seeds, k))
                 for k in range(n)]
        for party in (0, 1):
            assert_batches_equal(got[party], host[party], f"n={n} party {party}")
            assert_batch_equals_oracle(got[party], P, [o[party] for o in okeys], f"n={n}")
        if n == 33:
            _check_point_function(dpf, levels, dev[0], dev[1], alphas, beta_of)
    assert H == got[0].num_hierarchy_levels


def test_fresh_root_seeds_differ_and_keys_are_a_point_function():
    levels = MIXED
    dpf = make(levels)
    rng = np.random.default_rng(9)
    alphas = _alphas(rng, 33, 20)
    betas = [7, (1 << 128) - 3, 0x1234]
    values = [leaves_value(vt, [b]) for (_, vt, _), b in zip(levels, betas)]
    a = dpf.generate_key_batch_to_device(alphas, values)
    b = dpf.generate_key_batch_to_device(alphas, values)
    sa = np.concatenate([dpf.download_key_batch(d).seeds() for d in a])
    sb = np.concatenate([dpf.download_key_batch(d).seeds() for d in b])
    assert len({tuple(r) for r in np.concatenate([sa, sb]).tolist()}) == 4 * 33
    _check_point_function(dpf, levels, a[0], a[1], alphas, lambda k, h: betas[h])


def test_unsupported_value_types_fall_back_to_the_host():
    vt = ("tuple", [("intmodn", 32, G.M32)] * 2)
    levels = [(8, vt, 64.0), (16, vt, 64.0)]   # the heavy-hitters value type
    dpf = make(levels)
    assert not dpf.generates_keys_on_device()
    rng = np.random.default_rng(2)
    n = 33
    alphas = _alphas(rng, n, 16)
    seeds = seeds_array(rng, n)
    values = [leaves_value(vt, [1, 1]), leaves_value(vt, [2, 3])]
    host = dpf.generate_key_batch(alphas, values, root_seeds=seeds)
    dev = dpf.generate_key_batch_to_device(alphas, values, root_seeds=seeds)
    for party in (0, 1):
        assert_batches_equal(dpf.download_key_batch(dev[party]), host[party])


def test_129_hierarchy_levels_fall_back_to_the_host():
    """Log domains 0..128 are valid parameters with more hierarchy levels than
    the kernel's tables hold: the keys are generated on the host."""
    levels = [(i, ("int", 64), 0) for i in range(129)]
    dpf = make(levels)
    assert not dpf.generates_keys_on_device()
    rng = np.random.default_rng(129)
    n = 33
    alphas = _alphas(rng, n, 128)
    seeds = seeds_array(rng, n)
    betas = [int(b) for b in rng.integers(1, 1 << 62, size=129)]
    values = [leaves_value(("int", 64), [b]) for b in betas]
    host = dpf.generate_key_batch(alphas, values, root_seeds=seeds)
    dev = dpf.generate_key_batch_to_device(alphas, values, root_seeds=seeds)
    for party in (0, 1):
        assert_batches_equal(dpf.download_key_batch(dev[party]), host[party], f"party {party}")
    _check_point_function(dpf, levels, dev[0], dev[1], alphas, lambda k, h: betas[h],
                          only=(0, 64, 128))


@pytest.mark.parametrize("log", [6, 7], ids=["L4", "L5"])
def test_unaligned_control_arrays(log):
    """The C ABI takes any uint8_t* for cw_left and cw_right.  With L = 4 every
    control store of an aligned base is one dword and none of an offset base
    is; with L = 5 the keys alternate.  Every array of every placement equals
    the host batch, and nothing outside the arrays is written."""
    from distributed_point_functions_amd import hip_abi
    from keygen_common import gen_into_arena
    import torch
    hip_abi.load(require_gpu=True)
    levels = [(log, ("int", 32), 0)]
    P = O.OracleParams(levels)
    assert P.tree_levels_needed - 1 == log - 2
    dpf = make(levels)
    rng = np.random.default_rng(log)
    n = 33
    alphas = _alphas(rng, n, log)
    seeds = seeds_array(rng, n)
    beta = (1 << 32) - 1
    host = dpf.generate_key_batch(alphas, [leaves_value(("int", 32), [beta])], root_seeds=seeds)
    want = batch_arrays(host[0])
    for name in ("cw_seed", "cw_left", "cw_right", "vc0"):   # both parties hold the same
        np.testing.assert_array_equal(batch_arrays(host[1])[name], want[name])
    d_alphas = hip_abi.to_device_blocks(D.u128_array(alphas))
    d_seeds = hip_abi.to_device_blocks(seeds)
    d_beta = hip_abi.to_device_blocks(D.u128_array([beta]))
    for fill, (left, right) in zip((0xAB, 0x54, 0xC3, 0x3C), ((0, 0), (1, 2), (2, 3), (3, 1))):
        arena = gen_into_arena(hip_abi, P, n, d_alphas, d_seeds, d_beta, 0, fill,
                               offsets={"cw_left": left, "cw_right": right})
        torch.cuda.synchronize()
        assert arena.tensor("cw_left").data_ptr() % 4 == left
        assert arena.tensor("cw_right").data_ptr() % 4 == right
        assert_arrays_equal(arena.arrays(), want, f"offsets {left}, {right}")


def test_generation_and_evaluation_share_a_stream_without_a_sync():
    import torch
    levels = [(20, ("int", 64), 0)]
    dpf = make(levels)
    rng = np.random.default_rng(4)
    n = 513
    alphas = _alphas(rng, n, 20)
    seeds = seeds_array(rng, n)
    values = [leaves_value(levels[0][1], [77])]
    pts = _dev_points(alphas)
    torch.cuda.synchronize()   # the points are ready before either stream reads them
    outs = []
    for stream in (torch.cuda.Stream(), None):
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(None)
        with ctx:
            dev = dpf.generate_key_batch_to_device(alphas, values, root_seeds=seeds, stream=stream)
            res = []
            for d in dev:
                out = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
                dpf.evaluate_at_batch_to_device(d, 0, pts, 1, out, stream=stream)
                res.append(out)
        torch.cuda.synchronize()
        outs.append([r.cpu().numpy().view(np.uint64) for r in res])
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][0] + outs[0][1], np.full(n, 77, np.uint64))


# ---------------------------------------------------------------- DCF
@pytest.mark.parametrize("vt", [("int", 64), ("int", 128), ("xor", 64)], ids=str)
@pytest.mark.parametrize("n", [1, 2, 8, 64, 128])
def test_dcf_device_batches(n, vt):
    import torch
    dcf = make_dcf(vt, n)
    assert dcf.generates_keys_on_device()
    P = O.dcf_params(n, vt)
    kind, bits, _ = O.leaves(vt)[0]
    rng = np.random.default_rng(n * 3 + bits)
    keys = 33
    alphas = _alphas(rng, keys, n)
    betas = [[_beta_leaf(vt, k, rng)] for k in range(keys)]
    seeds = seeds_array(rng, keys)
    values = [leaves_value(vt, b) for b in betas]
    dev = dcf.generate_key_batch_to_device(alphas, values, root_seeds=seeds)
    got = [dcf.download_key_batch(d) for d in dev]
    single = [dcf.generate_keys(alphas[k], values[k], *seed_ints(seeds, k)) for k in range(keys)]
    okeys = [O.dcf_generate_keys(P, alphas[k], betas[k], *seed_ints(seeds, k)) for k in range(keys)]
    for party in (0, 1):
        assert_batches_equal(got[party], dcf.make_key_batch([s[party] for s in single]),
                             f"party {party}")
        assert_batch_equals_oracle(got[party], P, [o[party] for o in okeys], f"party {party}")
    # One beta for every key takes the same path.
    one = dcf.generate_key_batch_to_device(alphas, values[2:3], root_seeds=seeds)
    host_one = dcf.generate_key_batch(alphas, values[2:3], root_seeds=seeds)
    for party in (0, 1):
        assert_batches_equal(dcf.download_key_batch(one[party]), host_one[party])
    # x -> beta if x < alpha else 0, from the device-generated keys.
    top = (1 << n) - 1
    xs = [x for a in alphas for x in (0, (a - 1) & top, a, (a + 1) & top, top)]
    size = dcf.packed_size()
    ys = []
    for d in dev:
        out = torch.empty(keys * 5 * size, dtype=torch.uint8, device="cuda")
        assert dcf.evaluate_batch_to_device(d, _dev_points(xs), 5, out) == keys * 5
        torch.cuda.synchronize()
        ys.append(_ints(out.cpu().numpy(), size))
    for k in range(keys):
        for j in range(5):
            x, a, b = xs[5 * k + j], ys[0][5 * k + j], ys[1][5 * k + j]
            if kind == O.LEAF_XOR or n == 128:
                # SetToZero leaves an XorWrapper alone, and at n = 128 Evaluate takes
                # prefix 0 at every level: whatever the oracle's keys give.
                if k < 2:
                    want = O.add_packed(vt, O.dcf_evaluate(P, okeys[k][0], x),
                                        O.dcf_evaluate(P, okeys[k][1], x))
                    got = a ^ b if kind == O.LEAF_XOR else (a + b) % (1 << bits)
                    assert got == int.from_bytes(bytes(want[0]), "little"), (k, j)
            else:
                assert (a + b) % (1 << bits) == (betas[k][0] if x < alphas[k] else 0), (k, j)


# ---------------------------------------------------------------- MIC
@pytest.mark.parametrize("n", [8, 64])
def test_mic_device_batches(n):
    import torch
    N = 1 << n
    intervals = [(0, 3), (5, N // 2), (N - 2, N - 1)]
    m = len(intervals)
    g = M.MultipleIntervalContainmentGate.create(M.make_parameters(n, intervals))
    rng = np.random.default_rng(n)
    big = lambda: int.from_bytes(rng.bytes(16), "little") % N   # noqa: E731
    gates = 33
    r_in = [0, N - 1] + [big() for _ in range(gates - 2)]
    r_out = [[big() for _ in intervals] for _ in range(gates)]
    z_0 = [[big() for _ in intervals] for _ in range(gates)]
    seeds = seeds_array(rng, gates)
    dev = g.gen_batch_to_device(r_in, r_out, root_seeds=seeds, z_0=z_0)
    single = [g.gen(r_in[k], r_out[k], *seed_ints(seeds, k), z_0[k]) for k in range(gates)]
    for party in (0, 1):
        got = g.download_key_batch(dev[party])
        want = g.make_key_batch([s[party] for s in single])
        assert got.num_intervals == m
        np.testing.assert_array_equal(got.mask_shares(), want.mask_shares())
        assert_batches_equal(got.dcf(), want.dcf(), f"party {party}")
    # Masked inputs x + r_in: the shares recombine to the containment bits.
    x = [0, 3, 4, N - 1] + [big() for _ in range(gates - 4)]
    masked = [(x[k] + r_in[k]) % N for k in range(gates)]
    dx = torch.from_numpy(MM.u128_rows(masked).view(np.int64)).cuda()
    ys = []
    for d in dev:
        out = torch.zeros(gates * m * 16, dtype=torch.uint8, device="cuda")
        assert g.eval_batch_to_device(d, dx, out) == gates * m
        torch.cuda.synchronize()
        ys.append(MM.ints_of(out.cpu().numpy()))
    for k in range(gates):
        a, b = ys[0][k * m:(k + 1) * m], ys[1][k * m:(k + 1) * m]
        assert MM.reconstruct(n, a, b, r_out[k]) == MM.contains(intervals, x[k]), k
