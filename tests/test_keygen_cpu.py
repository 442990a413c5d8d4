"""Batched key generation, the parts that need no GPU: the two C ABI entry
points' argument checks, and the host generators behind the device ones --
DistributedPointFunction.generate_key_batch_with_betas, the DCF's
generate_key_batch and the MIC gate's gen_batch -- whose row k must be exactly
the single-key generation with the same root seeds (and the CPU oracle's)."""
import ctypes

import numpy as np
import pytest

import mic_model as MM
import oracle as O
import ref_grids as G
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import mic as M
from keygen_common import (EDGE_LEVELS, KeygenArena, assert_arrays_equal,
                           assert_batch_equals_oracle, assert_batches_equal, batch_arrays,
                           boundary_key_pairs, oracle_arrays, rows_of, seed_ints)
from test_dcf_cpu import make as make_dcf
from test_host_api_cpu import leaves_value
from test_key_batch_cpu import make, seeds_array

HIER = [(4, ("int", 32), 0), (6, ("int", 32), 0), (8, ("int", 32), 0)]
WIDE = [(128, ("int", 64), 0)]
MOD2 = ("tuple", [("intmodn", 32, G.M32)] * 2)


# ---------------------------------------------------------------- C ABI
def test_header_declares_and_library_exports_the_entry_points():
    lib = hip_abi.load()
    for name in ("dpf_hip_gen_key_batch", "dpf_hip_gen_keys_supported"):
        assert name in hip_abi.header_functions()
        assert hasattr(lib, name)


def _desc(vt, blocks=1):
    return hip_abi.value_desc(O.leaves(vt), O.is_direct(vt), O.elements_per_block(vt), blocks)


@pytest.mark.parametrize("bits", [8, 16, 32, 64, 128])
def test_gen_keys_supported_for_integers_and_xor_wrappers(bits):
    lib = hip_abi.load()
    for kind in ("int", "xor"):
        assert lib.dpf_hip_gen_keys_supported(ctypes.byref(_desc((kind, bits)))) == 1


def test_gen_keys_not_supported_for_int_mod_n_and_tuples():
    lib = hip_abi.load()
    assert lib.dpf_hip_gen_keys_supported(ctypes.byref(_desc(("intmodn", 32, G.M32)))) == 0
    assert lib.dpf_hip_gen_keys_supported(ctypes.byref(_desc(MOD2, 2))) == 0
    assert lib.dpf_hip_gen_keys_supported(None) == 0


def _gen_args(vt=("int", 64), **over):
    """Arguments of a one-level log-domain-1 call; every device pointer NULL."""
    I32 = ctypes.c_int32 * 1
    a = dict(num_keys=1, num_levels=0, H=1, tree_level=I32(0), log_domain=I32(1), blocks=I32(1),
             desc=ctypes.byref(_desc(vt)), alphas=None, root_seeds=None, beta=None, beta_mode=0,
             dcf_bits=0, kl=None, kr=None, kv=None, cw_seed=None, cw_left=None, cw_right=None,
             vc=None, stream=None)
    a.update(over)
    return list(a.values())


def test_gen_key_batch_checks_arguments_without_a_device():
    lib = hip_abi.load()
    assert lib.dpf_hip_gen_key_batch(*_gen_args(num_keys=0)) == 0
    assert lib.dpf_hip_gen_key_batch(*_gen_args()) == 3          # NULL outputs and inputs
    assert lib.dpf_hip_gen_key_batch(*_gen_args(num_levels=-1)) == 3
    assert lib.dpf_hip_gen_key_batch(*_gen_args(num_keys=-1)) == 3
    assert lib.dpf_hip_gen_key_batch(*_gen_args(beta_mode=7)) == 3
    assert lib.dpf_hip_gen_key_batch(*_gen_args(vt=("intmodn", 32, G.M32))) == 12
    assert b"value type" in lib.dpf_hip_last_error()


# ---------------------------------------------------------------- DPF
def _alphas(rng, n, top):
    fixed = [0, (1 << top) - 1, ((1 << 127) | (1 << 70) | 5) & ((1 << top) - 1)]
    rand = [int.from_bytes(rng.bytes(16), "little") & ((1 << top) - 1) for _ in range(n)]
    return (fixed + rand)[:n]


def _per_key_betas(levels, n, rng):
    """[key][level] leaves: 0, the all-ones value and random ones."""
    out = []
    for k in range(n):
        row = []
        for _, vt, _ in levels:
            bits = O.leaves(vt)[0][1]
            v = [0, (1 << bits) - 1][k] if k < 2 else int.from_bytes(rng.bytes(16), "little") % (1 << bits)
            row.append([v])
        out.append(row)
    return out


@pytest.mark.parametrize("levels", [HIER, WIDE] + [lv for lv, _ in EDGE_LEVELS],
                         ids=["hier", "log128"] + [f"edge{i}" for i in range(len(EDGE_LEVELS))])
def test_with_betas_rows_equal_single_keygen_and_oracle(levels):
    """The host generator on HIER, WIDE and the level-table edges of
    keygen_common.EDGE_LEVELS (the device tests of those lean on this batch);
    the alphas 0 and all ones have bit 127 clear and set."""
    dpf = make(levels)
    P = O.OracleParams(levels)
    for lv, tree in EDGE_LEVELS:
        if lv == levels:
            assert dpf.hierarchy_to_tree() == tree == list(P.hierarchy_to_tree)
    rng = np.random.default_rng(levels[-1][0])
    n = 9
    alphas = _alphas(rng, n, levels[-1][0])
    betas = _per_key_betas(levels, n, rng)
    seeds = seeds_array(rng, n)
    values = [leaves_value(vt, betas[k][h]) for k in range(n) for h, (_, vt, _) in enumerate(levels)]
    b0, b1 = dpf.generate_key_batch_with_betas(alphas, values, root_seeds=seeds, threads=2)
    okeys = []
    for k in range(n):
        s = seed_ints(seeds, k)
        row = values[k * len(levels):(k + 1) * len(levels)]
        k0, k1 = dpf.generate_keys_incremental(alphas[k], row, seeds=s)
        assert dpf.key_from_batch(b0, k).SerializeToString() == k0.SerializeToString()
        assert dpf.key_from_batch(b1, k).SerializeToString() == k1.SerializeToString()
        okeys.append(O.generate_keys(P, alphas[k], betas[k], *s))
    assert_batch_equals_oracle(b0, P, [o[0] for o in okeys], "party 0")
    assert_batch_equals_oracle(b1, P, [o[1] for o in okeys], "party 1")


def test_with_identical_betas_equals_generate_key_batch():
    dpf = make(HIER)
    rng = np.random.default_rng(5)
    n = 300   # two host threads' slices
    alphas = [int(x) for x in rng.integers(0, 256, size=n)]
    seeds = seeds_array(rng, n)
    beta = [leaves_value(vt, [h + 3]) for h, (_, vt, _) in enumerate(HIER)]
    shared = dpf.generate_key_batch(alphas, beta, root_seeds=seeds, threads=2)
    per_key = dpf.generate_key_batch_with_betas(alphas, beta * n, root_seeds=seeds, threads=2)
    for a, b in zip(shared, per_key):
        assert_batches_equal(b, a)


def test_generators_share_generate_key_batchs_errors():
    dpf = make(HIER)
    beta = [leaves_value(vt, [1]) for _, vt, _ in HIER]
    for gen, good in ((dpf.generate_key_batch, beta),
                      (dpf.generate_key_batch_with_betas, beta * 2)):
        with pytest.raises(D.DpfStatusError, match="`beta` has to have the same size as `parameters`"):
            gen([1, 2], good[:-1])
        with pytest.raises(D.DpfStatusError, match="`alpha` must be smaller than the output domain"):
            gen([1, 256], good)
        with pytest.raises(D.DpfStatusError, match="root_seeds must be empty or hold two seeds per"):
            gen([1, 2], good, root_seeds=np.zeros((3, 2), np.uint64))


# ---------------------------------------------------------------- test helpers
def _filled_arena(batch, fill, offsets=None):
    """A CPU arena holding the correction words of a host batch."""
    import torch
    want = batch_arrays(batch)
    H = batch.num_hierarchy_levels
    elements = [len(want[f"vc{h}"]) // batch.num_keys for h in range(H)]
    arena = KeygenArena(batch.num_keys, batch.num_levels, elements, fill, device="cpu",
                        offsets=offsets)
    for name in arena.spans:
        arena.tensor(name).copy_(torch.from_numpy(np.ascontiguousarray(want[name]).view(np.uint8)
                                                  .reshape(-1)))
    return arena, want


@pytest.mark.parametrize("offsets", [None, {"cw_left": 3, "cw_right": 1}], ids=["aligned", "offset"])
def test_arena_comparison_and_gap_check_can_fail(offsets):
    """The comparisons of the device tests on a CPU tensor: the arena's arrays
    equal the batch they were filled from, by name; one flipped byte in any one
    array fails the comparison; one byte written into any gap, before the first
    array or into the guard fails the gap check."""
    dpf = make(HIER)
    rng = np.random.default_rng(11)
    n = 5
    beta = [leaves_value(vt, [h + 3]) for h, (_, vt, _) in enumerate(HIER)]
    batch = dpf.generate_key_batch(_alphas(rng, n, 8), beta, root_seeds=seeds_array(rng, n))[0]
    arena, want = _filled_arena(batch, 0xAB, offsets)
    assert set(arena.spans) == set(want) - {"seed", "party"}
    assert_arrays_equal(arena.arrays(), want)
    starts = sorted(s for s, _ in arena.spans.values())
    ends = sorted(s + nb for s, nb in arena.spans.values())
    assert starts[0] >= KeygenArena.GAP
    assert all(a - b >= KeygenArena.GAP for a, b in zip(starts[1:], ends))
    assert arena.size - ends[-1] >= KeygenArena.GAP + KeygenArena.GUARD
    for name, (start, nbytes) in arena.spans.items():
        rel = (0 if offsets is None else offsets.get(name, 0))
        assert (arena.raw.data_ptr() + arena.base + start) % 16 == rel, name
        # A flipped byte: the first, the last.
        for at in (0, nbytes - 1):
            t = arena.tensor(name)
            t[at] ^= 1
            with pytest.raises(AssertionError, match=name):
                assert_arrays_equal(arena.arrays(), want)
            t[at] ^= 1
        # A byte written next to the array, on either side.
        for at in (start - 1, start + nbytes, start + nbytes + KeygenArena.GAP - 1):
            cell = arena.raw[arena.base + at:arena.base + at + 1]
            cell.fill_(0x54)
            with pytest.raises(AssertionError, match="outside the arrays"):
                arena.arrays()
            cell.fill_(0xAB)
    for at in (0, arena.size - KeygenArena.GUARD, arena.size - 1):
        cell = arena.raw[arena.base + at:arena.base + at + 1]
        cell.fill_(0)
        with pytest.raises(AssertionError, match="outside the arrays"):
            arena.arrays()
        cell.fill_(0xAB)
    assert_arrays_equal(arena.arrays(), want)
    # A missing or an extra array fails too.
    less = {k: v for k, v in arena.arrays().items() if k != "vc1"}
    with pytest.raises(AssertionError):
        assert_arrays_equal(less, want)


def test_rows_of_picks_the_oracles_keys():
    levels = EDGE_LEVELS[4][0]
    dpf = make(levels)
    P = O.OracleParams(levels)
    rng = np.random.default_rng(3)
    n = 9
    alphas = _alphas(rng, n, 5)
    betas = _per_key_betas(levels, n, rng)
    seeds = seeds_array(rng, n)
    values = [leaves_value(vt, betas[k][h]) for k in range(n) for h, (_, vt, _) in enumerate(levels)]
    b0, _ = dpf.generate_key_batch_with_betas(alphas, values, root_seeds=seeds)
    ks = [0, 4, 8]
    okeys = [O.generate_keys(P, alphas[k], betas[k], *seed_ints(seeds, k))[0] for k in ks]
    assert_arrays_equal(rows_of(batch_arrays(b0), ks, n), oracle_arrays(P, okeys))
    with pytest.raises(AssertionError):
        assert_arrays_equal(rows_of(batch_arrays(b0), [0, 4, 7], n), oracle_arrays(P, okeys))


@pytest.mark.parametrize("cus", [256, 304, 80])
def test_boundary_key_pairs(cus, monkeypatch):
    """At the key generation cases' size on a chip of `cus` compute units: the
    pairs are those of _boundary_items' lanes, at most 48, with the first, the
    last, the whole cut-off chunk and both sides of a workgroup boundary."""
    import test_dynamic_chunks_gpu as C
    monkeypatch.setattr(C, "_cus", lambda: cus)
    T = 4 * cus * 1024
    K = T // 2 + 113
    chunks = -(-2 * K // 64)
    assert chunks == T // 64 + 4 and 2 * K % 64 == 34
    per_wg = -(-chunks // cus)
    lanes = C._boundary_items(2 * K, per_wg)
    got = boundary_key_pairs(K, per_wg)
    assert got == sorted(set(got)) and len(got) <= 48
    assert set(got) <= {u // 2 for u in lanes}
    assert got[0] == 0 and got[-1] == K - 1
    assert set(range(K - 17, K)) <= set(got)          # the last chunk's 34 lanes
    span = per_wg * 64 // 2
    assert {span - 1, span} <= set(got)
    owners = -(-chunks // per_wg)
    assert any((owners - 1) * span <= k < K - 17 for k in got)
    # A tighter limit keeps the same pairs and samples fewer of the rest.
    few = boundary_key_pairs(K, per_wg, limit=24)
    assert len(few) == 24 and set(few) <= {u // 2 for u in lanes}
    assert set(range(K - 17, K)) | {0, span - 1, span} <= set(few)
    # A short list is returned whole.
    assert boundary_key_pairs(K, per_wg, limit=10 ** 6) == sorted({u // 2 for u in lanes})


# ---------------------------------------------------------------- DCF
@pytest.mark.parametrize("vt,n", [(("int", 64), 1), (("int", 64), 8), (("int", 64), 64),
                                  (("xor", 64), 8), (MOD2, 5)], ids=str)
def test_dcf_batch_rows_equal_single_keygen_and_oracle(vt, n):
    dcf = make_dcf(vt, n)
    # The tuple of IntModN pins the host path's zeroing of every leaf kind
    # against the single-key generation alone.
    P = None if vt == MOD2 else O.dcf_params(n, vt)
    rng = np.random.default_rng(n)
    keys = 6
    alphas = _alphas(rng, keys, n)
    nl = len(O.leaves(vt))
    betas = [[(1 << 64) - 1 if k == 1 and vt != MOD2 else 40 + k] * nl for k in range(keys)]
    seeds = seeds_array(rng, keys)
    b0, b1 = dcf.generate_key_batch(alphas, [leaves_value(vt, b) for b in betas],
                                    root_seeds=seeds, threads=2)
    single = [dcf.generate_keys(alphas[k], leaves_value(vt, betas[k]), *seed_ints(seeds, k))
              for k in range(keys)]
    assert_batches_equal(b0, dcf.make_key_batch([s[0] for s in single]), "party 0")
    assert_batches_equal(b1, dcf.make_key_batch([s[1] for s in single]), "party 1")
    if P is not None:
        okeys = [O.dcf_generate_keys(P, alphas[k], betas[k], *seed_ints(seeds, k))
                 for k in range(keys)]
        assert_batch_equals_oracle(b0, P, [o[0] for o in okeys], "party 0")
        assert_batch_equals_oracle(b1, P, [o[1] for o in okeys], "party 1")
    # One beta for all keys is the same as that beta repeated.
    one = dcf.generate_key_batch(alphas, [leaves_value(vt, betas[0])], root_seeds=seeds)
    rep = dcf.generate_key_batch(alphas, [leaves_value(vt, betas[0])] * keys, root_seeds=seeds)
    for a, b in zip(one, rep):
        assert_batches_equal(a, b)


def test_dcf_xor_wrapper_beta_is_not_zeroed():
    # SetToZero leaves an XorWrapper as it is (distributed_comparison_function.cc:21-32):
    # with alpha = 0 every level would take zero, yet the keys are those of beta.
    vt, n = ("xor", 64), 8
    dcf = make_dcf(vt, n)
    seeds = seeds_array(np.random.default_rng(1), 1)
    with_beta = dcf.generate_key_batch([0], [leaves_value(vt, [0xABCD])], root_seeds=seeds)[0]
    with_zero = dcf.generate_key_batch([0], [leaves_value(vt, [0])], root_seeds=seeds)[0]
    a, b = batch_arrays(with_beta), batch_arrays(with_zero)
    assert any(not np.array_equal(a[f"vc{h}"], b[f"vc{h}"]) for h in range(n))
    P = O.dcf_params(n, vt)
    okey = O.dcf_generate_keys(P, 0, [0xABCD], *seed_ints(seeds, 0))[0]
    assert_batch_equals_oracle(with_beta, P, [okey])


def test_dcf_batch_errors():
    dcf = make_dcf(("int", 64), 8)
    with pytest.raises(D.DpfStatusError, match="`alpha` must be smaller than the output domain"):
        dcf.generate_key_batch([1, 256], [5])
    with pytest.raises(D.DpfStatusError, match="root_seeds must be empty or hold two seeds per"):
        dcf.generate_key_batch([1, 2], [5], root_seeds=np.zeros((2, 2), np.uint64))
    with pytest.raises(D.DpfStatusError, match="one value or one per alpha"):
        dcf.generate_key_batch([1, 2, 3], [5, 6])


# ---------------------------------------------------------------- MIC
@pytest.mark.parametrize("n", [8, 64])
def test_mic_gen_batch_equals_per_key_gen(n):
    N = 1 << n
    intervals = [(0, 3), (5, N // 2), (N - 2, N - 1)]
    g = M.MultipleIntervalContainmentGate.create(M.make_parameters(n, intervals))
    rng = np.random.default_rng(n)
    big = lambda: int.from_bytes(rng.bytes(16), "little") % N   # noqa: E731
    gates = 5
    r_in = [0, N - 1] + [big() for _ in range(gates - 2)]
    r_out = [[big() for _ in intervals] for _ in range(gates)]
    z_0 = [[big() for _ in intervals] for _ in range(gates)]
    seeds = seeds_array(rng, gates)
    b0, b1 = g.gen_batch(r_in, r_out, root_seeds=seeds, z_0=z_0)
    single = [g.gen(r_in[k], r_out[k], *seed_ints(seeds, k), z_0[k]) for k in range(gates)]
    for got, party in ((b0, 0), (b1, 1)):
        want = g.make_key_batch([s[party] for s in single])
        assert got.num_intervals == want.num_intervals == len(intervals)
        np.testing.assert_array_equal(got.mask_shares(), want.mask_shares())
        assert_batches_equal(got.dcf(), want.dcf(), f"party {party}")
    # Fresh randomness: the shares still add up to the corrected masks.
    f0, f1 = g.gen_batch(r_in, r_out)
    s = [(a + b) % N for a, b in zip(MM.ints_of(f0.mask_shares()), MM.ints_of(f1.mask_shares()))]
    assert s == [(a + b) % N for a, b in zip(MM.ints_of(b0.mask_shares()), MM.ints_of(b1.mask_shares()))]
    assert not np.array_equal(f0.dcf().seeds(), b0.dcf().seeds())


def test_mic_gen_batch_errors_are_gen_impls():
    g = M.MultipleIntervalContainmentGate.create(M.make_parameters(8, [(0, 3), (5, 9)]))
    with pytest.raises(D.DpfStatusError, match="Count of output masks should be equal to the number of intervals"):
        g.gen_batch([1, 2], [[1, 2], [3]])
    with pytest.raises(D.DpfStatusError, match="Input mask should be between 0 and 2\\^log_group_size"):
        g.gen_batch([256], [[1, 2]])
    with pytest.raises(D.DpfStatusError, match="Output mask should be between 0 and 2\\^log_group_size"):
        g.gen_batch([1], [[1, 256]])
    with pytest.raises(D.DpfStatusError, match="Count of mask shares should be equal to the number of output masks"):
        g.gen_batch([1], [[1, 2]], z_0=[[1]])
