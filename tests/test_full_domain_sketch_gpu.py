"""Checked private histograms on an MI355X (dpf_hip_expand_sketch through
evaluate_full_domain_sum_sketch_to_device, hip_abi.expand_sketch and
histogram.py): the field sums and every key's sketches against the CPU oracle's
per-key EvaluateUntil rows, reduced with Python integers and
tests/sketch_model.py.  Both maps are exact modular arithmetic, independent of
order: every comparison is an equality."""
import functools

import numpy as np
import pytest

import oracle as O
import sketch_model as M
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import heavy_hitters as HH
from distributed_point_functions_amd import hip_abi
from distributed_point_functions_amd import histogram as HG
from distributed_point_functions_amd import proto as pb
from keygen_common import seed_ints
from test_host_api_cpu import leaves_value
from test_key_batch_cpu import make, seeds_array

pytestmark = pytest.mark.gpu

M32 = (1 << 32) - 5      # shift 0
M17 = 65537              # shift 15
HH_VT = ("tuple", [("intmodn", 32, M32)] * 2)
TYPES = [("intmodn", 32, M32), ("intmodn", 32, M17), HH_VT, ("tuple", [("intmodn", 32, M17)] * 2)]
KEYS = (1, 63, 64, 65, 130)
DOMAINS = (1, 2, 3, 6, 10)
HOOK = "DPF_EXPAND_SKETCH_WAVE_ITEMS"
POISON = -0x54545455     # 0xAB bytes


def _dev_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _weights(rng, J, n, N):
    """J rows of n 32-bit weights with 0, N - 1, N and 2^32 - 1 among them."""
    w = rng.integers(0, 1 << 32, size=(J, n), dtype=np.uint64)
    special = [0, N - 1, N, (1 << 32) - 1]
    for j in range(J):
        for i in range(min(n, 4)):
            w[j, i] = special[(i + j) % 4]
    return w.astype(np.uint32)


def _run(dpf, dev, h, n, nl, w=None, accumulate=False, out=None):
    """(sums uint32 [2^n, nl], sketches uint32 [K, J, nl]) through the device
    call; a fresh sum buffer and the sketch buffer are poisoned."""
    import torch
    J = 0 if w is None else w.shape[0]
    if out is None:
        out = torch.full((1 << n, nl), POISON, dtype=torch.int32, device="cuda")
    sk = torch.full((dev.num_keys, J, nl), POISON, dtype=torch.int32, device="cuda")
    got = dpf.evaluate_full_domain_sum_sketch_to_device(h, dev, w, out, sk if J else None,
                                                        accumulate=accumulate)
    assert got == 1 << n
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).copy(), sk.cpu().numpy().view(np.uint32).copy()


def _mod_sum(rows, mods):
    """rows: uint32 [K][N][nl] -> uint32 [N][nl], summed in Python integers."""
    s = np.asarray(rows).astype(object).sum(axis=0)
    return (s % np.array(mods, dtype=object)).astype(np.uint32)


def _betas(mods, k):
    """Leaves 0, 1 and N_e - 1 (and others) over the keys."""
    return [(0, 1, N - 1, 7, (k * 2654435761) % N)[(k + e) % 5] for e, N in enumerate(mods)]


# ---- 1. the shape grid against the oracle -------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(type_index, n):
    """130 keys of both parties from host key generation with fixed root seeds,
    the oracle's full-domain rows of each, and the models of the sums of the
    first K keys and of every key's sketches under two weight rows: computed
    once per (type, domain)."""
    vt = TYPES[type_index]
    levels = [(n, vt, 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    mods = M.moduli(vt)
    nl, N, K = len(mods), 1 << n, max(KEYS)
    rng = np.random.default_rng(n * 7 + nl + mods[0] % 11)
    alphas = [0, N - 1, N // 2, 1 % N] + [int(a) for a in rng.integers(0, N, size=K - 4)]
    betas = [_betas(mods, k) for k in range(K)]
    seeds = seeds_array(rng, K)
    host = dpf.generate_key_batch_with_betas(alphas, [leaves_value(vt, b) for b in betas],
                                             root_seeds=seeds)
    w = _weights(rng, 2, N, mods[0])
    rows, sketches = [], []
    for party in (0, 1):
        ys = []
        for k in range(K):
            okey = O.generate_keys(P, alphas[k], [betas[k]], *seed_ints(seeds, k))[party]
            ys.append(np.ascontiguousarray(O.evaluate_until(P, 0, [], O.create_context(P, okey))))
        packed = np.stack(ys).reshape(K, -1)
        rows.append(packed.view("<u4").reshape(K, N, nl).copy())
        sketches.append(M.sketch(vt, packed, w))
    return dpf, host, alphas, betas, mods, w, rows, sketches


def _schedules(K):
    """The plan's default (at these shapes the deepest walk, no stack), nothing
    walked (the whole tree on the depth-first stack, one atomic per sketch
    accumulator) and walk == 2 wherever the tree has the levels (four subtrees
    per chunk)."""
    return (None, "1", str(4 * -(-K // 64)))


@pytest.mark.parametrize("n", DOMAINS)
@pytest.mark.parametrize("vt", TYPES, ids=lambda v: str(v)[:34])
def test_oracle_parity_over_the_shape_grid(vt, n, monkeypatch):
    """K in {1, 63, 64, 65, 130} (partial and several chunks, clamped lanes) of
    both parties, J in {0, 1, 2}, three schedules each; n = 1 is exactly one
    leaf pair, n = 2 one level above it, n = 10 a stack nine deep."""
    dpf, host, alphas, betas, mods, w, rows, sketches = _case(TYPES.index(vt), n)
    assert dpf.evaluates_full_domain_sum_sketch_on_device(0)
    nl = len(mods)
    dw = _dev_u32(w)
    cus = _cus()
    shares = {}
    for party in (0, 1):
        for K in KEYS:
            dev = dpf.upload_key_batch(host[party], 0, K)
            want_sum = _mod_sum(rows[party][:K], mods)
            walks = set()
            for hook in _schedules(K):
                if hook is None:
                    monkeypatch.delenv(HOOK, raising=False)
                else:
                    monkeypatch.setenv(HOOK, hook)
                walks.add(hip_abi.expand_sketch_plan(K, n, cus)["walk"])
                for J in (2, 1, 0):
                    got_sum, got_sk = _run(dpf, dev, 0, n, nl, dw[:J] if J else None)
                    msg = f"party {party} K {K} J {J} hook {hook}"
                    np.testing.assert_array_equal(got_sum, want_sum, err_msg=msg)
                    np.testing.assert_array_equal(got_sk, sketches[party][:K, :J], err_msg=msg)
            assert walks == {0, min(2, n - 1), n - 1}, (K, walks)
            shares[party, K] = want_sum
    monkeypatch.delenv(HOOK, raising=False)
    # The two parties' sums reconstruct the plaintext histogram mod N_e.
    hist = np.zeros((1 << n, nl), dtype=object)
    for a, b in zip(alphas, betas):
        hist[a] += np.array(b, dtype=object)
    hist = (hist % np.array(mods, dtype=object)).astype(np.uint32)
    np.testing.assert_array_equal(HG.reconstruct_mod(shares[0, 130], shares[1, 130], mods), hist)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 2. the item loop -------------------------------------------------------------------
def test_dynamic_and_static_item_loops_agree(monkeypatch):
    """65 keys (two chunks, the second one key) with the threshold hook at
    chunked_shape's rule -- 4 chunks for each of the 16 waves of one workgroup
    per CU, here wave items: the same bytes with the loop dynamic (default) and
    with DPF_EXPAND_SKETCH_DYNAMIC=0, each run reporting its own loop; keys 0,
    63 and 64 equal the oracle's model."""
    cus, K, vt = _cus(), 65, HH_VT
    rule = cus * 16 * 4
    n = next(n for n in range(3, 22) if 2 << (n - 2) >= rule)   # one level left for the stack
    monkeypatch.setenv(HOOK, str(rule))
    pl = hip_abi.expand_sketch_plan(K, n, cus)
    assert pl["wave_items"] >= rule and 0 < pl["walk"] < n - 1
    levels = [(n, vt, 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    rng = np.random.default_rng(5)
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=K)]
    seeds = seeds_array(rng, K)
    host = dpf.generate_key_batch(alphas, [leaves_value(vt, [1, 7])], root_seeds=seeds)
    w = _weights(rng, 2, 1 << n, M32)
    dw = _dev_u32(w)
    devs = [dpf.upload_key_batch(b) for b in host]
    outs = []
    for hook, dynamic in ((None, True), ("0", False)):
        if hook is None:
            monkeypatch.delenv("DPF_EXPAND_SKETCH_DYNAMIC", raising=False)
        else:
            monkeypatch.setenv("DPF_EXPAND_SKETCH_DYNAMIC", hook)
        outs.append(_run(dpf, devs[0], 0, n, 2, dw))
        assert (hip_abi.last_dynamic_chunks() > 0) == dynamic, (n, hook)
    monkeypatch.delenv("DPF_EXPAND_SKETCH_DYNAMIC", raising=False)
    assert outs[0][0].tobytes() == outs[1][0].tobytes()
    assert outs[0][1].tobytes() == outs[1][1].tobytes()
    for k in (0, 63, 64):
        okey = O.generate_keys(P, alphas[k], [[1, 7]], *seed_ints(seeds, k))[0]
        y = np.ascontiguousarray(O.evaluate_until(P, 0, [], O.create_context(P, okey)))
        np.testing.assert_array_equal(outs[0][1][k], M.sketch(vt, y.reshape(1, -1), w)[0],
                                      err_msg=f"key {k}")
    other, sk1 = _run(dpf, devs[1], 0, n, 2, dw)
    hist = np.zeros((1 << n, 2), dtype=np.uint32)
    for a in alphas:
        hist[a] += np.array([1, 7], dtype=np.uint32)
    np.testing.assert_array_equal(HG.reconstruct_mod(outs[0][0], other, [M32, M32]), hist)


# ---- 3. the weights -------------------------------------------------------------------------
@pytest.mark.parametrize("vt", [("intmodn", 32, M17), HH_VT], ids=lambda v: str(v)[:34])
def test_weight_edges(vt):
    """All 0, all 2^32 - 1 (>= N: reduced first), all N - 1, and random."""
    n = 6
    dpf, host, alphas, betas, mods, w, rows, sketches = _case(TYPES.index(vt), n)
    nl, N, K = len(mods), 1 << n, 130
    rng = np.random.default_rng(6)
    sets = np.stack([np.zeros(N, np.uint32), np.full(N, (1 << 32) - 1, np.uint32),
                     np.full(N, mods[0] - 1, np.uint32),
                     rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)])
    dev = dpf.upload_key_batch(host[1])
    packed = rows[1].reshape(K, -1).view(np.uint8)
    for pair in ((0, 1), (2, 3)):
        wj = sets[list(pair)]
        got_sum, got_sk = _run(dpf, dev, 0, n, nl, _dev_u32(wj))
        np.testing.assert_array_equal(got_sk, M.sketch(vt, packed, wj), err_msg=str(pair))
        np.testing.assert_array_equal(got_sum, _mod_sum(rows[1], mods))
        if pair == (0, 1):
            assert not got_sk[:, 0].any()


# ---- 4. accumulate, overwrite and the empty batch ---------------------------------------------
@pytest.mark.parametrize("vt", [("intmodn", 32, M17), HH_VT], ids=lambda v: str(v)[:34])
def test_accumulate_and_overwrite(vt):
    import torch
    n = 6
    dpf, host, alphas, betas, mods, w, rows, sketches = _case(TYPES.index(vt), n)
    nl, N, K = len(mods), 1 << n, 130
    dw = _dev_u32(w)
    whole = dpf.upload_key_batch(host[0])
    want = _mod_sum(rows[0], mods)
    # Overwriting reads nothing of what the buffer held.
    a, sk_a = _run(dpf, whole, 0, n, nl, dw)
    b, _ = _run(dpf, whole, 0, n, nl, dw, out=torch.zeros((N, nl), dtype=torch.int32, device="cuda"))
    np.testing.assert_array_equal(a, want)
    assert a.tobytes() == b.tobytes()
    # Two batches into one sum, the second starting from entries equal to
    # N_e - 1 (a wrap of the modular add), its sketches those of its own keys.
    first, second = dpf.upload_key_batch(host[0], 0, 70), dpf.upload_key_batch(host[0], 70, K)
    top = np.broadcast_to(np.array(mods, dtype=np.uint32) - 1, (N, nl))
    out = _dev_u32(top).reshape(N, nl).clone()
    got, sk2 = _run(dpf, second, 0, n, nl, dw, accumulate=True, out=out)
    want2 = _mod_sum([top, _mod_sum(rows[0][70:], mods)], mods)
    np.testing.assert_array_equal(got, want2)
    np.testing.assert_array_equal(sk2, sketches[0][70:])
    got, sk1 = _run(dpf, first, 0, n, nl, dw, accumulate=True, out=out)
    np.testing.assert_array_equal(got, _mod_sum([top, want], mods))
    np.testing.assert_array_equal(sk1, sketches[0][:70])      # overwritten, not accumulated
    halves, _ = _run(dpf, first, 0, n, nl, dw)
    halves, _ = _run(dpf, second, 0, n, nl, dw, accumulate=True, out=_dev_u32(halves).reshape(N, nl))
    np.testing.assert_array_equal(halves, want)
    # The empty batch: zeros, or the buffer as it was; no kernel is launched.
    empty = dpf.upload_key_batch(host[0], 0, 0)
    assert empty.num_keys == 0
    z, sk0 = _run(dpf, empty, 0, n, nl, dw)
    assert not z.any() and sk0.shape == (0, 2, nl)
    kept, _ = _run(dpf, empty, 0, n, nl, dw, accumulate=True)
    assert (kept.view(np.int32) == POISON).all()
    # The host-returning call equals the device call; J = 0 is the plain sum.
    s, k = dpf.evaluate_full_domain_sum_sketch(0, whole, w)
    np.testing.assert_array_equal(s, want)
    np.testing.assert_array_equal(k, sk_a)
    s, k = dpf.evaluate_full_domain_sum_sketch(0, whole)
    np.testing.assert_array_equal(s, want)
    assert k.shape == (K, 0, nl)
    s, k = dpf.evaluate_full_domain_sum_sketch(0, empty, w)
    assert not s.any() and s.shape == (N, nl) and k.shape == (0, 2, nl)


# ---- 5. the hierarchy -------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0, 1])
def test_both_levels_of_an_incremental_dpf_match_the_oracle(h):
    levels = [(4, ("intmodn", 32, M32), 0), (9, HH_VT, 0)]
    dpf = make(levels)
    P = O.OracleParams(levels)
    n, vt = levels[h][0], levels[h][1]
    mods = M.moduli(vt)
    nl, N, K = len(mods), 1 << n, 70
    rng = np.random.default_rng(40 + h)
    alphas = [int(a) for a in rng.integers(0, 1 << 9, size=K)]
    seeds = seeds_array(rng, K)
    betas = [[11], [1, 7]]
    host = dpf.generate_key_batch(alphas, [leaves_value(levels[i][1], betas[i]) for i in (0, 1)],
                                  root_seeds=seeds)
    w = _weights(rng, 2, N, mods[0])
    shares = []
    for party in (0, 1):
        got_sum, got_sk = _run(dpf, dpf.upload_key_batch(host[party]), h, n, nl, _dev_u32(w))
        ys = []
        for k in range(K):
            okey = O.generate_keys(P, alphas[k], betas, *seed_ints(seeds, k))[party]
            ys.append(np.ascontiguousarray(O.evaluate_until(P, h, [], O.create_context(P, okey))))
        packed = np.stack(ys).reshape(K, -1)
        np.testing.assert_array_equal(got_sum, _mod_sum(packed.view("<u4").reshape(K, N, nl), mods),
                                      err_msg=f"party {party}")
        np.testing.assert_array_equal(got_sk, M.sketch(vt, packed, w), err_msg=f"party {party}")
        shares.append(got_sum)
    hist = np.zeros((N, nl), dtype=np.uint32)
    for a in alphas:
        hist[a >> (9 - n)] += np.array(betas[h], dtype=np.uint32)
    np.testing.assert_array_equal(HG.reconstruct_mod(shares[0], shares[1], mods), hist)


# ---- 6. two different moduli, at the C ABI ------------------------------------------------------
def _sample(block0, next_word, mods):
    """The sampling of a tuple of IntModN<uint32_t, N_e> from the hashed blocks
    (value_type_helpers.h:415-443, int_mod_n.h:155-177) in Python integers."""
    r, out = block0, []
    for e, N in enumerate(mods):
        out.append(r % N)
        r = (((r // N) << 32) | next_word[e]) & ((1 << 128) - 1) if e + 1 < len(mods) else 0
    return out


def _model_rows(key, n, mods, corr, party):
    """One key's full domain from the oracle's tree expansion and value hash,
    sampled, corrected and negated here: uint32 [2^n][nl]."""
    cs, cl, cr = O._cw_arrays(key, 0, n)
    seeds, ctrl = O.expand_seeds(O.blocks_from_ints([key["seed"]]), np.array([key["party"]], np.uint8),
                                 cs, cl, cr)
    ints = O.ints_from_blocks(seeds)
    h0 = O.ints_from_blocks(O.aes_hash(O.PRG_KEY_VALUE, seeds))
    h1 = O.ints_from_blocks(O.aes_hash(O.PRG_KEY_VALUE, O.blocks_from_ints(
        [(s + 1) & O.MASK128 for s in ints])))
    rows = np.zeros((1 << n, len(mods)), dtype=np.uint32)
    for i in range(1 << n):
        x = _sample(h0[i], [h1[i] & 0xFFFFFFFF], mods)
        for e, N in enumerate(mods):
            v = (x[e] + corr[e]) % N if ctrl[i] else x[e]
            rows[i, e] = (N - v) % N if party else v
    return rows


@pytest.mark.parametrize("mods", [(M32, M32), (M32, M17), (M17, M32)], ids=str)
def test_two_moduli_at_the_c_abi(mods):
    """The DPF object, like the reference, takes tuples of one modulus only;
    dpf_hip_expand_sketch takes any two, which catches a leaf or modulus index
    mix-up.  Trees of oracle keys, value corrections of this test's choosing
    (N_e - 1 among them); the model above equals the oracle's own rows for the
    heavy-hitters type (first case)."""
    import torch
    n, K = 5, 66
    N = 1 << n
    levels = [(n, HH_VT, 0)]
    P = O.OracleParams(levels)
    rng = np.random.default_rng(sum(mods) % 1000)
    keys, corrs, rows = [], [], []
    for k in range(K):
        s0, s1 = (int(x) for x in rng.integers(1, 1 << 62, size=2))
        pair = O.generate_keys(P, int(rng.integers(0, N)), [[1, 7]], s0, s1)
        key = pair[k & 1]
        corr = list(key["last_vc"][0]) if mods == (M32, M32) else \
            [m - 1 if k % 3 == 0 else int(rng.integers(0, m)) for m in mods]
        keys.append(key)
        corrs.append(corr)
        rows.append(_model_rows(key, n, mods, corr, k & 1))
        if mods == (M32, M32) and k < 4:
            y = np.ascontiguousarray(O.evaluate_until(P, 0, [], O.create_context(P, key)))
            np.testing.assert_array_equal(rows[-1], y.view("<u4").reshape(N, 2))
    desc = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 32, m) for m in mods], False, 1, 2)
    cw = [O._cw_arrays(key, 0, n) for key in keys]
    w = _weights(rng, 2, N, mods[0])
    got_sum, got_sk = hip_abi.expand_sketch(
        n, hip_abi.to_device_blocks(O.blocks_from_ints([key["seed"] for key in keys])),
        hip_abi.to_device_u8([key["party"] for key in keys]),
        hip_abi.to_device_blocks(np.stack([c[0] for c in cw])),
        hip_abi.to_device_u8(np.stack([c[1] for c in cw])),
        hip_abi.to_device_u8(np.stack([c[2] for c in cw])),
        (O.PRG_KEY_LEFT, O.PRG_KEY_RIGHT, O.PRG_KEY_VALUE), desc,
        hip_abi.to_device_blocks(O.blocks_from_ints([c for corr in corrs for c in corr])),
        weights=_dev_u32(w))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got_sum.cpu().numpy().view(np.uint32), _mod_sum(rows, mods))
    want_sk = np.zeros((K, 2, 2), dtype=np.uint32)
    for e, m in enumerate(mods):
        y = np.stack(rows)[:, :, e].astype(object)
        want_sk[:, :, e] = (np.dot(w.astype(object) % m, y.T) % m).T.astype(np.uint32)
    np.testing.assert_array_equal(got_sk.cpu().numpy().view(np.uint32), want_sk)


# ---- 7. the protocol, end to end through histogram.py ---------------------------------------------
E2E_N, E2E_CLIENTS, E2E_SEED = 8, 130, 2026
BAD_VALUE, BAD_BIT, BAD_BIN = 5, 64, 129


def _tampered(ser, alphas):
    """Three malformed clients: a value correction with one leaf changed (in
    both servers' keys: beta is no longer (1, 7)), the last level's control-bit
    correction flipped in one server's key, and -- the lose side's control-bit
    correction flipped in both keys, so that alpha's sibling stays on the path
    -- a second nonzero bin."""
    def edit(party, k, fn):
        key = pb.DpfKey.FromString(ser[party][k])
        fn(key)
        ser[party][k] = key.SerializeToString()

    def leaf(key):
        v = key.last_level_value_correction[0].tuple.elements[1].int_mod_n
        v.value_uint64 = (v.value_uint64 + 1) % M32

    def left(key):
        cw = key.correction_words[-1]
        cw.control_left = not cw.control_left

    def lose(key):
        cw = key.correction_words[-1]
        if alphas[BAD_BIN] & 1:
            cw.control_left = not cw.control_left
        else:
            cw.control_right = not cw.control_right

    for party in (0, 1):
        edit(party, BAD_VALUE, leaf)
        edit(party, BAD_BIN, lose)
    edit(1, BAD_BIT, left)


def test_histogram_reconstructs_and_flags_malformed_clients():
    """130 honest clients reconstruct the plaintext histogram mod N and all
    pass `check`; with three keys tampered in the same batch those three are
    flagged and the honest ones still pass.  N = 2^32 - 5: a malformed vector
    passes with probability about 2^-31 over the weights; the seeds are fixed."""
    import torch
    n, K = E2E_N, E2E_CLIENTS
    N = 1 << n
    dpf = make([(n, HH_VT, 0)])
    rng = np.random.default_rng(E2E_SEED)
    alphas = [int(a) for a in rng.integers(0, N, size=K)]
    host = dpf.generate_key_batch(alphas, [D.to_value(HH.value_type(), HH.BETA)],
                                  root_seeds=seeds_array(rng, K))
    w = HH.sketch_weights(E2E_SEED, 0, N)
    hist = np.zeros((N, 2), dtype=np.uint32)
    for a in alphas:
        hist[a] += np.array(HH.BETA, dtype=np.uint32)
    folds = [HG.fold_checked(dpf, dpf.upload_key_batch(b), w) for b in host]
    torch.cuda.synchronize()
    (s0, k0), (s1, k1) = folds
    assert s0.shape == (N, 2) and k0.shape == (K, 2, 2) and s0.dtype == torch.int32
    np.testing.assert_array_equal(HG.reconstruct_mod(s0, s1, [M32, M32]), hist)
    assert HG.check(k0, k1).all()
    # J = 0: the plain field sum, streamed in as two batches.
    plain, none = HG.fold_checked(dpf, dpf.upload_key_batch(host[0], 0, 64), None, accumulate=True)
    HG.fold_checked(dpf, dpf.upload_key_batch(host[0], 64, K), None, out=plain, accumulate=True)
    torch.cuda.synchronize()
    assert none.shape == (64, 0, 2)
    np.testing.assert_array_equal(plain.cpu().numpy(), s0.cpu().numpy())
    # The same batch with three tampered keys.
    ser = [dpf.serialize_key_batch(b) for b in host]
    _tampered(ser, alphas)
    devs = [dpf.upload_key_batch(dpf.parse_key_batch(s)) for s in ser]
    (t0, b0), (t1, b1) = [HG.fold_checked(dpf, d, w) for d in devs]
    torch.cuda.synchronize()
    ok = HG.check(b0, b1)
    assert sorted(np.flatnonzero(~ok).tolist()) == [BAD_VALUE, BAD_BIT, BAD_BIN]
    # The third client's own vector has exactly two nonzero bins: alpha and its sibling.
    one = [dpf.upload_key_batch(dpf.parse_key_batch([s[BAD_BIN]])) for s in ser]
    y = HG.reconstruct_mod(HG.fold_checked(dpf, one[0], None)[0],
                           HG.fold_checked(dpf, one[1], None)[0], [M32, M32])
    assert sorted(np.flatnonzero(y.any(axis=1)).tolist()) == sorted(
        [alphas[BAD_BIN], alphas[BAD_BIN] ^ 1])
    np.testing.assert_array_equal(y[alphas[BAD_BIN]], np.array(HH.BETA, dtype=np.uint32))


# ---- 8. no regression ------------------------------------------------------------------------------
def test_full_domain_sum_still_refuses_the_field_type():
    import torch
    dpf = make([(6, HH_VT, 0)])
    d0 = dpf.upload_key_batch(
        dpf.generate_key_batch([3, 5], [D.to_value(HH.value_type(), HH.BETA)])[0])
    out = torch.zeros(1 << 7, dtype=torch.int64, device="cuda")
    with pytest.raises(D.DpfStatusError, match="UNIMPLEMENTED.*uint64_t and XorWrapper<uint64_t>"):
        dpf.evaluate_full_domain_sum_to_device(d0, 0, out)
    assert not out.cpu().numpy().any()
    assert not dpf.evaluates_full_domain_sum_on_device(0)
    assert dpf.evaluates_full_domain_sum_sketch_on_device(0)
