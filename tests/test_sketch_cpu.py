"""The sketch check of the heavy-hitters driver on the CPU
(heavy_hitters.sketch_weights / check_sketches) and the linearity of the
sketch model (tests/sketch_model.py) on the oracle's two-party outputs."""
import numpy as np

import oracle as O
import sketch_model as M
from distributed_point_functions_amd import heavy_hitters as HH

N = HH.MODULUS
VT = ("tuple", [("intmodn", 32, N)] * 2)


def test_sketch_weights_deterministic_and_squared():
    a = HH.sketch_weights(11, 3, 1000)
    b = HH.sketch_weights(11, 3, 1000)
    assert a.dtype == np.uint32 and a.shape == (2, 1000)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, HH.sketch_weights(11, 4, 1000))
    assert not np.array_equal(a, HH.sketch_weights(12, 3, 1000))
    assert int(a.max()) < N
    r = [int(x) for x in a[0]]
    assert [int(x) for x in a[1]] == [x * x % N for x in r]


def _shares(vec, w, rng):
    """Additive shares mod N of the sketch of `vec` ((n, 2) ints) under w."""
    z = np.array([[sum(int(w[j][i]) * int(vec[i][e]) for i in range(len(vec))) % N
                   for e in range(2)] for j in range(2)], dtype=object)
    s0 = np.array(rng.integers(0, N, size=(2, 2)), dtype=object)
    s1 = (z - s0) % N
    return s0.astype(np.uint32), s1.astype(np.uint32)


def test_check_sketches_accepts_unit_and_zero_rejects_the_rest():
    rng = np.random.default_rng(5)
    n = 64
    w = HH.sketch_weights(7, 0, n)
    zero = [[0, 0] for _ in range(n)]
    unit = [list(z) for z in zero]
    unit[17] = [HH.BETA[0], HH.BETA[1]]
    two = [list(z) for z in unit]
    two[40] = [HH.BETA[0], HH.BETA[1]]
    scale2 = [list(z) for z in zero]
    scale2[17] = [2 * HH.BETA[0], 2 * HH.BETA[1]]
    wrong_tag = [list(z) for z in zero]
    wrong_tag[17] = [HH.BETA[0], HH.BETA[1] + 1]
    vecs = [unit, zero, two, scale2, wrong_tag]
    sh = [_shares(v, w, rng) for v in vecs]
    s0 = np.stack([a for a, _ in sh])
    s1 = np.stack([b for _, b in sh])
    assert HH.check_sketches(s0, s1).tolist() == [True, True, False, False, False]


def test_model_is_linear_on_the_oracles_two_party_outputs():
    levels = [(4, VT, HH.SECURITY_PARAMETER), (6, VT, HH.SECURITY_PARAMETER)]
    P = O.OracleParams(levels)
    alpha = 0b101101
    k0, k1 = O.generate_keys(P, alpha, [list(HH.BETA)] * 2, 1234567, 7654321)
    c0, c1 = O.create_context(P, k0), O.create_context(P, k1)
    for h, prefixes in ((0, []), (1, [alpha >> 2, 3])):
        y0 = O.evaluate_until(P, h, prefixes, c0)
        y1 = O.evaluate_until(P, h, prefixes, c1)
        n = y0.shape[0]
        w = HH.sketch_weights(3, h, n)
        s = M.sketch(VT, np.stack([y0, y1]), w)
        z = (s[0].astype(np.uint64) + s[1].astype(np.uint64)) % np.uint64(N)
        vals = HH.output_values(prefixes, 2, n)
        i_star = vals.index(alpha >> (6 - levels[h][0]))
        for j in range(2):
            for e in range(2):
                assert int(z[j][e]) == int(w[j][i_star]) * HH.BETA[e] % N
        assert HH.check_sketches(s[0:1], s[1:2]).tolist() == [True]
