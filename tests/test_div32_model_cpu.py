"""The Python-int model of the mod-N division (tests/div32_model.py) against
`%` and `//`, and the coverage conditions of tests/test_mod32_moduli_gpu.py.

The coverage conditions are conditions, not measurements: for every GPU case
that claims a branch of div_2by1, the case's own census -- computed here from
the CPU oracle's hashed value blocks and the model, nothing else -- shows the
branch reached at every leaf position claimed.  A kernel whose copy of the
division loses the second correction, or applies the first unconditionally,
then stores a wrong residue in that case.
"""
import random

import pytest

import div32_cases as C
import div32_model as M

U32 = (1 << 32) - 1


# ---- 1. the model is the arithmetic ---------------------------------------------------------
@pytest.mark.parametrize("N", C.GRID, ids=hex)
def test_div_2by1_equals_divmod(N):
    d = M.make_div32(N)
    assert d.dn == N << d.sh and d.dn >> 31 == 1 and d.v == ((1 << 64) - 1) // d.dn - (1 << 32)
    rnd = random.Random(N)
    cases = [(u1, u0) for u1 in (0, 1, d.dn - 1) for u0 in (0, 1, U32)]
    cases += [(rnd.randrange(d.dn), rnd.randrange(1 << 32)) for _ in range(20000)]
    for u1, u0 in cases:
        q, r, _ = M.div_2by1(u1, u0, d.dn, d.v)
        assert (q, r) == divmod((u1 << 32) | u0, d.dn), (u1, u0)


@pytest.mark.parametrize("N", C.GRID, ids=hex)
def test_divmod128_equals_divmod_and_keeps_96_quotient_bits(N):
    d = M.make_div32(N)
    rnd = random.Random(N + 1)
    blocks = [w3 << 96 | rest for w3 in (d.dn - 1, d.dn & U32, U32, 0, 1)
              for rest in (0, (1 << 96) - 1, rnd.getrandbits(96))]
    blocks += [rnd.getrandbits(128) for _ in range(5000)]
    blocks += [rnd.getrandbits(32) << 96 | rnd.getrandbits(rnd.randrange(1, 97))
               for _ in range(1000)]
    for x in blocks:
        r, q, steps = M.divmod128(M.words(x), d)
        assert r == x % N, hex(x)
        assert q[0] | q[1] << 32 | q[2] << 64 == (x // N) & ((1 << 96) - 1), hex(x)
        assert len(steps) == (3 if d.sh == 0 else 4)


@pytest.mark.parametrize("N", C.GRID, ids=hex)
def test_mod32_mul_mod_mod64_equal_percent(N):
    d = M.make_div32(N)
    rnd = random.Random(N + 2)
    for x in [0, 1, N - 1, N, min(N + 1, U32), U32] + [rnd.getrandbits(32) for _ in range(5000)]:
        assert M.mod32(x, d)[0] == x % N, x
    pairs = [(a, y) for a in (0, 1, N - 1) for y in (0, 1, N - 1, N, U32)]
    pairs += [(rnd.randrange(N), rnd.getrandbits(32)) for _ in range(5000)]
    pairs += [(rnd.randrange(N), rnd.randrange(N)) for _ in range(5000)]
    pairs += list(C.mul_mod_pairs(N)) if N in C.SECOND else []
    for a, y in pairs:
        assert M.mul_mod(a, y, d)[0] == a * y % N, (a, y)
    sums = [0, 1, N - 1, N, U32, 1 << 32, (1 << 64) - 1, (N - 1) * 257, U32 * U32]
    sums += [rnd.getrandbits(rnd.randrange(1, 65)) for _ in range(5000)]
    for s in sums:
        assert M.mod64(s, d)[0] == s % N, s


@pytest.mark.parametrize("N", C.GRID, ids=hex)
@pytest.mark.parametrize("nl", [1, 2, 5])
def test_tuple_sampling_equals_the_rule(N, nl):
    rnd = random.Random(N + nl)
    for _ in range(500):
        block, nxt = rnd.getrandbits(128), [rnd.getrandbits(32) for _ in range(5)]
        vals, steps = M.sample(block, nxt, [N] * nl)
        assert vals == M.sample_reference(block, nxt, [N] * nl)
        assert len(steps) == nl
    # two different moduli: each leaf position divides by its own
    mods = [N, 65537, C.P32, 17, N][:max(nl, 2)]
    for _ in range(200):
        block, nxt = rnd.getrandbits(128), [rnd.getrandbits(32) for _ in range(5)]
        assert M.sample(block, nxt, mods)[0] == M.sample_reference(block, nxt, mods)


def test_a_residue_without_the_second_correction_is_off_by_n():
    """What a kernel without the second correction returns from mul_mod is the
    residue plus N: congruent, so a sum of such products reduced by mod64
    still comes out right.  That is why dpf_hip_sketch_rows cannot tell a
    mul_mod without its second correction from a whole one (mod64's own second
    correction is out of reach, see the table below), while an unconditional
    first correction (`exposed`) gives a residue that is NOT congruent."""
    for N in C.SECOND:
        d = M.make_div32(N)
        for a, y in C.mul_mod_pairs(N):
            p = (a * y) << d.sh
            q, r, s = M.div_2by1(p >> 32, p & U32, d.dn, d.v)
            assert s.second
            without = r + d.dn                 # the remainder before `rr -= d`
            assert without <= U32 and without >> d.sh == a * y % N + N
            if s.exposed:                      # first forced: rr + d wraps, nothing undoes it
                forced = (r + d.dn + d.dn) & U32
                assert forced < d.dn and (forced >> d.sh) % N != a * y % N


# ---- 2. which branches random inputs reach, per helper and modulus ------------------------
# (first correction both ways, second correction) over 20000 fixed-seed draws.
# mod64's sums are what the kernels can hold at test sizes: below 2^44 (a row
# of 2^12 terms below 2^32).  mod32, and mod64 at these sums, reach the second
# correction for NO grid modulus: no test claims to cover it there.
NEVER, BOTH, ALWAYS = "never", "both", "always"
CENSUS_TABLE = {
    # helper: {modulus: (first, second reached)}
    "div_2by1": {C.P32: (ALWAYS, False), 0x80010001: (BOTH, True), 65537: (BOTH, True),
                 17: (BOTH, True), 1 << 31: (BOTH, False)},
    "divmod128": {C.P32: (ALWAYS, False), 0x80010001: (BOTH, True), 65537: (BOTH, True),
                  17: (BOTH, True), 1 << 31: (BOTH, False)},
    "mod32": {C.P32: (ALWAYS, False), 0x80010001: (BOTH, False), 65537: (BOTH, False),
              17: (BOTH, False), 1 << 31: (BOTH, False)},
    "mul_mod y < N": {C.P32: (ALWAYS, False), 0x80010001: (BOTH, True), 65537: (BOTH, False),
                      17: (BOTH, False), 1 << 31: (BOTH, False)},
    "mul_mod any y": {C.P32: (ALWAYS, False), 0x80010001: (BOTH, True), 65537: (BOTH, True),
                      17: (BOTH, True), 1 << 31: (BOTH, False)},
    "mod64 < 2^44": {C.P32: (ALWAYS, False), 0x80010001: (BOTH, False), 65537: (BOTH, False),
                     17: (BOTH, False), 1 << 31: (BOTH, False)},
}


def _random_census(helper, N, draws=20000):
    d = M.make_div32(N)
    rnd = random.Random(f"{helper}{N}")
    c = M.Census()
    for _ in range(draws):
        if helper == "div_2by1":
            c.add([M.div_2by1(rnd.randrange(d.dn), rnd.getrandbits(32), d.dn, d.v)[2]])
        elif helper == "divmod128":
            c.add(M.divmod128(M.words(rnd.getrandbits(128)), d)[2])
        elif helper == "mod32":
            c.add(M.mod32(rnd.getrandbits(32), d)[1])
        elif helper == "mul_mod y < N":
            c.add(M.mul_mod(rnd.randrange(1, N), rnd.randrange(1, N), d)[1])
        elif helper == "mul_mod any y":
            c.add(M.mul_mod(rnd.randrange(1, N), rnd.getrandbits(32), d)[1])
        else:
            # sums of up to 2^12 reduced products: s <= 2^12 (N - 1) < 2^44
            c.add(M.mod64(rnd.randrange(min(1 << 44, (N - 1) << 12) + 1), d)[1])
    return c


@pytest.mark.parametrize("helper", CENSUS_TABLE, ids=str)
@pytest.mark.parametrize("N", C.GRID, ids=hex)
def test_census_table(helper, N):
    c = _random_census(helper, N)
    first = ALWAYS if not c.skipped else NEVER if not c.first else BOTH
    assert (first, c.second > 0) == CENSUS_TABLE[helper][N], c
    # Wherever the second correction is reached, so is an input on which an
    # unconditional first correction stays wrong.
    assert (c.exposed > 0) == (c.second > 0), c


# ---- 3. the coverage conditions of the GPU cases ----------------------------------------------
@pytest.mark.parametrize("shape", C.EXPAND_SHAPES, ids=str)
@pytest.mark.parametrize("N", C.GRID, ids=hex)
@pytest.mark.parametrize("nl", C.EXPAND_LEAVES)
def test_expand_cases_reach_their_branches(shape, N, nl):
    census = C.expand_census(shape, N, nl)
    assert len(census) == nl and all(c.steps for c in census)
    assert C.check_claims([N] * nl, census, f"expand {shape}") == []


def test_expand_corrections_hit_the_wrap():
    """N - 1 is the correction of leaf 0 in every case; two leaves add 0 or a
    random value, five leaves have all of {0, 1, N - 1, random}."""
    for N in C.GRID:
        for party in (0, 1):
            for nl in C.EXPAND_LEAVES:
                (v,) = C.expand_corrections(N, nl, party)
                assert len(v) == nl and all(0 <= x < N for x in v) and v[0] == N - 1
            assert {0, 1, N - 1} < set(C.expand_corrections(N, 5, party)[0])


@pytest.mark.parametrize("N", C.BATCH_MODULI, ids=hex)
@pytest.mark.parametrize("nl", C.BATCH_LEAVES)
@pytest.mark.parametrize("sum_mode", [False, True], ids=["per_key", "sum"])
def test_batch_cases_reach_their_branches(N, nl, sum_mode):
    """The last level of the run: the one whose kernel the GPU test reads."""
    census = C.batch_census(N, nl, sum_mode)
    assert C.check_claims([N] * nl, census, "batch") == []


@pytest.mark.parametrize("N", C.BATCH_MODULI, ids=hex)
@pytest.mark.parametrize("nl", C.BATCH_LEAVES)
def test_fused_sketch_cases_reach_their_branches(N, nl):
    census = C.fused_census(N, nl)
    assert C.check_claims([N] * nl, census, "fused sketch") == []


@pytest.mark.parametrize("N", C.GRID, ids=hex)
def test_sketch_rows_cases_reach_their_branches(N):
    """mul_mod takes its second correction in every case of the moduli that
    reach it -- the single-entry rows included, which are directed pairs --
    and the first correction both ways at row_len 257; mod32 and mod64 never
    take the second (the table above)."""
    for K in C.SKETCH_K:
        for row_len in C.SKETCH_ROW_LEN:
            for J in C.SKETCH_J:
                c = C.sketch_rows_census(N, K, row_len, J)
                what = (hex(N), K, row_len, J, c)
                assert (c["mul_mod"].second > 0) == (N in C.SECOND), what
                assert (c["mul_mod"].exposed > 0) == (N in C.SECOND), what
                if row_len > 1:
                    assert c["mul_mod"].first > 0 and c["mod32"].both_ways(), what
                    assert (c["mul_mod"].skipped > 0) or N == C.P32, what
                assert c["mod32"].second == 0 and c["mod64"].second == 0, what
    if N == 0x80010001:
        d = M.make_div32(N)
        for a, y in C.mul_mod_pairs(N, 4, True):
            assert a < N and y < N and M.mul_mod(a, y, d)[1][0].second


def test_sketch_rows_hold_unreduced_entries_and_edge_weights():
    for N in C.GRID:
        y, w = C.sketch_rows_case(N, 70, 257, 4)
        ys, ws = set(y.reshape(-1).tolist()), set(w.reshape(-1).tolist())
        assert {min(N, U32), min(N + 1, U32), U32, N - 1, 0} <= ys
        assert {0, N - 1, N, U32} <= ws
        assert (y >= N).any()


@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("party", [0, 1])
def test_histogram_cases_reach_their_branches(nl, party):
    """The claim is made at n = 6 with 65 keys (64 leaves x 65 keys); the
    one-key and one-level shapes run the same code on too few leaves to claim
    anything."""
    census = C.hist_census(nl, 6, 65, party)
    assert C.check_claims([C.HIST_N] * nl, census, "histogram") == []
    betas = C.hist_case(nl, 6)[1]
    assert {0, 1, C.HIST_N - 1} <= {b for bs in betas for b in bs}


@pytest.mark.parametrize("mods", C.ABI_PAIRS, ids=str)
def test_two_moduli_cases_reach_their_branches(mods):
    assert C.check_claims(list(mods), C.abi_census(mods), "two moduli") == []
    _, corrs, _ = C.abi_case(mods)
    assert all(any(c[e] == m - 1 for c in corrs) for e, m in enumerate(mods))
