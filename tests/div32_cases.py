"""Fixed-seed inputs of tests/test_mod32_moduli_gpu.py, and the census of
div_2by1's corrections that each of them reaches (tests/div32_model.py).

The GPU tests import the builders; tests/test_div32_model_cpu.py imports the
same builders and proves, from the oracle and the model alone, that every case
which claims a branch reaches it at every leaf position.  A kernel's copy of
the sampling loop with a correction deleted or made unconditional then gives a
wrong residue in that case.

The modulus grid:
    2^32 - 5     shift 0; the first correction is always taken
    0x80010001   shift 0; reaches the second correction (in mul_mod too, with
                 reduced operands)
    65537        shift 15; reaches the second correction
    17           shift 27 (a wide normalisation shift); reaches the second
    2^31         a power of two, v = 2^32 - 1; never the second
"""
import functools

import numpy as np

import div32_model as M
import oracle as O

P32 = (1 << 32) - 5
GRID = (P32, 0x80010001, 65537, 17, 1 << 31)
SECOND = (0x80010001, 65537, 17)          # reach the second correction
BOTH_WAYS = (0x80010001, 65537, 1 << 31)  # take the first correction both ways
ALWAYS_FIRST = (P32,)                     # never skip the first correction
U32 = (1 << 32) - 1


def value_type(N, nl):
    return ("intmodn", 32, N) if nl == 1 else ("tuple", [("intmodn", 32, N)] * nl)


def check_claims(mods, census, what=""):
    """The coverage conditions of one case: census[e] belongs to modulus
    mods[e].  Returns the list of claims that do NOT hold (empty: all hold)."""
    missed = []
    for e, (N, c) in enumerate(zip(mods, census)):
        if N in SECOND and not (c.second > 0 and c.exposed > 0):
            missed.append(f"{what} leaf {e} N={N:#x}: second correction not reached: {c}")
        if N in BOTH_WAYS and not c.both_ways():
            missed.append(f"{what} leaf {e} N={N:#x}: first correction not both ways: {c}")
        if N in ALWAYS_FIRST and c.skipped:
            missed.append(f"{what} leaf {e} N={N:#x}: first correction skipped: {c}")
    return missed


# ---- 1. full-domain expansion (dpf_hip_expand) ---------------------------------------------
# shape -> (tree levels, start nodes)
EXPAND_SHAPES = {"small": (9, 1), "pair": (17, 3), "octet": (18, 5)}
EXPAND_LEAVES = (1, 2, 5)
EXPAND_SEC64 = 0x80010001        # the one modulus also run at security 40 and 64
CENSUS_LEAVES = 1024             # tree leaves the expansion census looks at


def expand_runs(shape, nl):
    """[(hooks, kernel dpf_hip_expand reports)] of a shape.  One workgroup
    takes the 2^9 tree; 3 x 2^17 leaves are still a small tree (192 workgroups
    of 11 levels), so the pair kernel is reached there with the small-tree
    launch switched off (and the octet kernel too, which one and two leaves
    would take: Mod32Leaf<2>); at 5 x 2^18 one and two leaves run the octet
    kernel, and the pair kernel with DPF_EXPAND_NO_OCTET=1, five leaves
    (Mod32Leaf<5>) the pair kernel."""
    no_octet = {"DPF_EXPAND_NO_OCTET": "1"}
    if shape == "small":
        return [({}, "small/mod32")]
    if shape == "pair":
        return [({}, "small/mod32"), (dict(no_octet, DPF_EXPAND_SMALL="0"), "pair/mod32")]
    return [({}, "pair/mod32")] if nl > 2 else [({}, "octet/mod32"), (no_octet, "pair/mod32")]


@functools.lru_cache(maxsize=None)
def expand_tree(shape):
    """Start seeds, control bits and correction words of a shape: one tree per
    shape, shared by every modulus and tuple length (the value hash, and so the
    census, depends on nothing else)."""
    levels, n0 = EXPAND_SHAPES[shape]
    rng = np.random.default_rng(1000 + levels * 8 + n0)
    return {"seeds": rng.integers(0, 2**64, size=(n0, 2), dtype=np.uint64),
            "ctrl": rng.integers(0, 2, size=n0, dtype=np.uint8),
            "cws": rng.integers(0, 2**64, size=(levels, 2), dtype=np.uint64),
            "cl": rng.integers(0, 2, size=levels, dtype=np.uint8),
            "cr": rng.integers(0, 2, size=levels, dtype=np.uint8)}


def expand_corrections(N, nl, party):
    """Value corrections from {N - 1, random, 0, 1}: N - 1 at leaf 0, so that
    the IntModN += wraps for N > 2^31 (and party 1 negates N - r); the other
    three follow in an order that depends on the party."""
    rnd = int(np.random.default_rng(N % 1009 + nl).integers(2, N - 1))
    pool = [N - 1, 0, 1, rnd] if party else [N - 1, rnd, 0, 1]
    return [[pool[e % 4] for e in range(nl)]]


def expand_inputs(shape, N, nl, party):
    return dict(expand_tree(shape), vcw=expand_corrections(N, nl, party))


@functools.lru_cache(maxsize=None)
def _expand_leaf_seeds(shape):
    t = expand_tree(shape)
    es, _ = O.expand_seeds(t["seeds"], t["ctrl"], t["cws"], t["cl"], t["cr"])
    return es[:CENSUS_LEAVES].copy()


def expand_census(shape, N, nl):
    """Per leaf position, over the first CENSUS_LEAVES tree leaves of the shape
    (a branch reached in a part of a case is reached in the case)."""
    return M.sampling_census(_expand_leaf_seeds(shape), [N] * nl)


# ---- 2. batched prefix evaluation (dpf_hip_prefix_batch_level) -----------------------------
BATCH_MODULI = (0x80010001, 65537)
BATCH_LEAVES = (2, 1)
BATCH_KEYS = {False: 70, True: 130}       # per key / summed over keys


def batch_levels(N, nl):
    """A heavy-hitters-shaped hierarchy: 2-bit steps, four levels from 4 bits."""
    vt = value_type(N, nl)
    return [(b, vt, 64.0) for b in (4, 6, 8, 10)], [0, 1, 2, 3]


def batch_seed(N, nl, n_keys):
    return N % 997 + 10 * nl + n_keys


def batch_census(N, nl, sum_mode):
    """Census of the LAST level of the run (the level whose kernel the test
    reads from last_batch_kernel), over all keys."""
    from test_batch_context_gpu import _prefix_plan
    from test_key_batch_gpu import _setup
    levels, plan = batch_levels(N, nl)
    n_keys = BATCH_KEYS[sum_mode]
    _, P, rng, _, oks, _, _, _ = _setup(levels, n_keys, seed=batch_seed(N, nl, n_keys))
    return _until_census_last(P, oks, _prefix_plan(P, plan, rng), [N] * nl)


def _until_census_last(P, oks, calls, mods):
    """Census of the last of `calls` = [(hierarchy level, prefixes)] over the
    oracle keys `oks`, from the seeds the oracle hashes into values; the
    earlier calls only move the contexts on."""
    out = [M.Census() for _ in mods]
    for key in oks:
        ctx = O.create_context(P, key)
        for h, prefixes in calls[:-1]:
            O.evaluate_until(P, h, prefixes, ctx)
        with M.recorded_value_seeds() as seen:
            O.evaluate_until(P, *calls[-1], ctx)
        for a, b in zip(out, M.sampling_census(np.concatenate(seen), mods)):
            a.merge(b)
    return out


# The fused per-key sketch (hh_keys_sketch): 70 keys, J = 2, prefixes without
# duplicates, so that every level after the first takes the fused kernel.
FUSED_KEYS = 70
FUSED_CALLS = [(0, []),
               (1, [9, 2, 14, 5]),
               (2, [(9 << 2) | 1, (2 << 2) | 3, (14 << 2) | 0, (5 << 2) | 2]),
               (3, [(37 << 2) | 3, (11 << 2) | 0, (56 << 2) | 2, (22 << 2) | 1])]


def fused_seed(N, nl):
    return N % 991 + nl


def fused_census(N, nl):
    from test_key_batch_gpu import _setup
    levels, _ = batch_levels(N, nl)
    _, P, _, _, oks, _, _, _ = _setup(levels, FUSED_KEYS, seed=fused_seed(N, nl))
    return _until_census_last(P, oks, FUSED_CALLS, [N] * nl)


# ---- 3. dpf_hip_sketch_rows ---------------------------------------------------------------
SKETCH_K = (1, 70)
SKETCH_ROW_LEN = (1, 257)
SKETCH_J = (1, 4)
SKETCH_NL = 2


@functools.lru_cache(maxsize=None)
def mul_mod_pairs(N, count=8, reduced=False):
    """(w, y) with w < N for which mul_mod(w, y) takes the second correction
    (and, every other pair, one for which an unconditional first correction
    would stay wrong), found by searching the model over a fixed stream.
    `reduced`: y < N as well."""
    d = M.make_div32(N)
    rng = np.random.default_rng(N % 1013)
    out, tries = [], 0
    while len(out) < count:
        tries += 1
        assert tries < 2_000_000, f"no mul_mod pair for N={N:#x}"
        w = int(rng.integers(0, N))
        y = int(rng.integers(0, N if reduced else 1 << 32))
        r, (s,) = M.mul_mod(w, y, d)
        assert r == w * y % N
        if s.second and (len(out) % 2 == 0 or s.exposed):
            out.append((w, y))
    return tuple(out)


def sketch_rows_case(N, K, row_len, J):
    """(y uint32 [K][row_len][2], w uint32 [J][row_len]): random 32-bit rows
    and weights -- the rows are NOT reduced: include/dpf_hip.h puts no bound on
    `in` -- with N, N + 1, 2^32 - 1, N - 1 and 0 among the row entries, 0,
    N - 1, N and 2^32 - 1 among the weights, and, for the moduli that reach
    it, directed (w, y) pairs that take mul_mod's second correction (for
    0x80010001 also pairs with y < N)."""
    rng = np.random.default_rng(N % 1019 + 1000 * K + 10 * row_len + J)
    y = rng.integers(0, 1 << 32, size=(K, row_len, SKETCH_NL), dtype=np.uint64)
    w = rng.integers(0, 1 << 32, size=(J, row_len), dtype=np.uint64)
    ys = [min(N, U32), min(N + 1, U32), U32, N - 1, 0]
    ws = [0, N - 1, N, U32]
    pairs = mul_mod_pairs(N) if N in SECOND else ()
    if N == 0x80010001:                    # with reduced operands as well
        pairs += mul_mod_pairs(N, 4, True)
    if row_len == 1:
        # one entry: a directed pair where there is one, else (N - 1) * (2^32 - 1)
        wy = pairs[1] if pairs else (N - 1, U32)
        w[:, 0] = wy[0]
        y[:, 0, :] = wy[1]
        if K > 1:
            y[1, 0, :] = U32
            y[2, 0, :] = min(N, U32)
    else:
        for i, v in enumerate(ys):
            y[:, i, (i + 1) % 2] = v
        for j in range(J):
            for i, v in enumerate(ws):
                w[j, (i + j) % 4] = v
        for i, (pw, py) in enumerate(pairs):
            w[i % J, 8 + i] = pw
            y[:, 8 + i, i % 2] = py
    return y.astype(np.uint32), w.astype(np.uint32)


def sketch_rows_census(N, K, row_len, J):
    """{"mod32", "mul_mod", "mod64"} -> Census of the whole case, the results
    checked against `%` on the way."""
    y, w = sketch_rows_case(N, K, row_len, J)
    d = M.make_div32(N)
    out = {"mod32": M.Census(), "mul_mod": M.Census(), "mod64": M.Census()}
    wr = []
    for j in range(J):
        row = []
        for x in w[j].tolist():
            r, s = M.mod32(x, d)
            assert r == x % N
            out["mod32"].add(s)
            row.append(r)
        wr.append(row)
    for k in range(min(K, 3)):             # three keys' rows say enough
        for e in range(SKETCH_NL):
            col = y[k, :, e].tolist()
            for j in range(J):
                total = 0
                for a, x in zip(wr[j], col):
                    r, s = M.mul_mod(a, x, d)
                    assert r == a * x % N
                    out["mul_mod"].add(s)
                    total += r
                r, s = M.mod64(total, d)
                assert r == total % N
                out["mod64"].add(s)
    return out


# ---- 4. checked histograms (dpf_hip_expand_sketch) -----------------------------------------
HIST_N = 0x80010001
HIST_DOMAINS = (1, 6)
HIST_KEYS = (1, 65)
HIST_J = 2


def weights(rng, J, n, N):
    """J rows of n 32-bit weights with 0, N - 1, N and 2^32 - 1 among them."""
    w = rng.integers(0, 1 << 32, size=(J, n), dtype=np.uint64)
    special = [0, N - 1, N, U32]
    for j in range(J):
        for i in range(min(n, 4)):
            w[j, i] = special[(i + j) % 4]
    return w.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def hist_case(nl, n):
    """65 keys of one level of 2^n bins of IntModN<0x80010001> (nl = 1) or its
    2-tuple: alphas, beta leaves (0, 1 and N - 1 among them), root seeds and
    two weight rows; a test takes the first K keys."""
    K, dom = max(HIST_KEYS), 1 << n
    rng = np.random.default_rng(7000 + 10 * n + nl)
    alphas = ([0, dom - 1, dom // 2, 1 % dom] + [int(a) for a in rng.integers(0, dom, size=K)])[:K]
    betas = [[(0, 1, HIST_N - 1, 7, (k * 2654435761) % HIST_N)[(k + e) % 5] for e in range(nl)]
             for k in range(K)]
    seeds = rng.integers(0, 1 << 63, size=(2 * K, 2), dtype=np.uint64)
    return alphas, betas, seeds, weights(rng, HIST_J, dom, HIST_N)


def seed_pair(seeds, k):
    s0 = int(seeds[2 * k, 0]) | int(seeds[2 * k, 1]) << 64
    s1 = int(seeds[2 * k + 1, 0]) | int(seeds[2 * k + 1, 1]) << 64
    return s0, s1


def hist_oracle_keys(nl, n, party):
    alphas, betas, seeds, _ = hist_case(nl, n)
    P = O.OracleParams([(n, value_type(HIST_N, nl), 0)])
    return P, [O.generate_keys(P, alphas[k], [betas[k]], *seed_pair(seeds, k))[party]
               for k in range(len(alphas))]


def hist_census(nl, n, K, party):
    _, keys = hist_oracle_keys(nl, n, party)
    return M.merged([M.key_census(key, n, [HIST_N] * nl) for key in keys[:K]])


# Two different moduli at the C ABI.
ABI_PAIRS = ((0x80010001, 65537), (65537, 0x80010001))
ABI_N, ABI_KEYS = 5, 66


@functools.lru_cache(maxsize=None)
def abi_case(mods):
    """66 oracle key trees of alternating parties with value corrections of
    this case's choosing (N_e - 1 every third key), and two weight rows."""
    dom = 1 << ABI_N
    P = O.OracleParams([(ABI_N, value_type(P32, 2), 0)])
    rng = np.random.default_rng(sum(mods) % 1000)
    keys, corrs = [], []
    for k in range(ABI_KEYS):
        s0, s1 = (int(x) for x in rng.integers(1, 1 << 62, size=2))
        keys.append(O.generate_keys(P, int(rng.integers(0, dom)), [[1, 7]], s0, s1)[k & 1])
        corrs.append([m - 1 if k % 3 == 0 else int(rng.integers(0, m)) for m in mods])
    return keys, corrs, weights(rng, 2, dom, mods[0])


def abi_census(mods):
    keys, _, _ = abi_case(mods)
    return M.merged([M.key_census(key, ABI_N, list(mods)) for key in keys])
