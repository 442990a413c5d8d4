"""MultipleIntervalContainmentGate on an MI355X (dpf_hip_mic_eval_batch):
bit-exact against the model (mic_model: Fig. 14 of eprint 2020/1392 over the
oracle's DCF) on the same keys, the reference's two Gen-and-Eval tests
(multiple_interval_containment_test.cc:37-208) by reconstruction, batches of
distinct keys in every launch shape, and a launch that fills the chip against
the same result composed from DistributedComparisonFunction's batched kernel."""
import numpy as np
import pytest

import mic_model as MM
from distributed_point_functions_amd import dcf as C
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import mic as M
from distributed_point_functions_amd import proto as pb
from test_mic_cpu import REF64, REF127, gate

pytestmark = pytest.mark.gpu


def run_batch(g, keys, xs, device_batch=None):
    """eval_batch_to_device of keys[i] at xs[i]: [gate][interval] Python ints."""
    import torch
    m = g.num_intervals()
    dev = device_batch if device_batch is not None else g.upload_key_batch(g.make_key_batch(keys))
    dx = torch.from_numpy(MM.u128_rows(xs).view(np.int64)).cuda()
    out = torch.zeros(max(len(keys) * m, 1) * 16, dtype=torch.uint8, device="cuda")
    assert g.eval_batch_to_device(dev, dx, out) == len(keys) * m
    torch.cuda.synchronize()
    flat = MM.ints_of(out.cpu().numpy()[:len(keys) * m * 16])
    return [flat[i * m:(i + 1) * m] for i in range(len(keys))]


def big(rng, N):
    return int.from_bytes(rng.bytes(16), "little") % N


class Case:
    """`gates` gates over one set of intervals, each with its own key pair."""

    def __init__(self, n, intervals, gates, seed):
        self.n, self.intervals, self.N = n, intervals, 1 << n
        self.g = gate(n, intervals)
        rng = np.random.default_rng(seed)
        m = len(intervals)
        self.r_in = [big(rng, self.N) for _ in range(gates)]
        self.r_out = [[big(rng, self.N) for _ in range(m)] for _ in range(gates)]
        self.z_0 = [[big(rng, self.N) for _ in range(m)] for _ in range(gates)]
        self.pairs = [self.g.gen(self.r_in[i], self.r_out[i], 2 * i + 1, 2 * i + 2, self.z_0[i])
                      for i in range(gates)]
        # Inputs at and around the bounds as well as anywhere.
        edges = [v for p, q in intervals for v in (p, q, p - 1, q + 1)] or [0]
        self.x = [(edges[int(rng.integers(0, len(edges)))] % self.N) if i % 3 else big(rng, self.N)
                  for i in range(gates)]
        self.masked = [(x + r) % self.N for x, r in zip(self.x, self.r_in)]

    def keys(self, flip=0):
        """Party (i + flip) % 2 of gate i."""
        return [self.pairs[i][(i + flip) % 2] for i in range(len(self.pairs))]

    def model_row(self, i, party):
        mk = MM.gen(self.n, self.intervals, self.r_in[i], self.r_out[i], 2 * i + 1, 2 * i + 2,
                    self.z_0[i])[party]
        return MM.evaluate(self.n, self.intervals, mk, self.masked[i])

    def check(self, model_gates):
        a = run_batch(self.g, self.keys(0), self.masked)
        b = run_batch(self.g, self.keys(1), self.masked)
        for i in range(len(self.pairs)):
            assert MM.reconstruct(self.n, a[i], b[i], self.r_out[i]) == \
                MM.contains(self.intervals, self.x[i]), f"gate {i}"
        for i in model_gates:
            assert a[i] == self.model_row(i, i % 2), f"gate {i}"
            assert b[i] == self.model_row(i, (i + 1) % 2), f"gate {i}"
        return a, b


def test_n5_all_inputs_one_batch():
    # q' wraps to 0, the full group, duplicate offsets (|U| = 6 for 10 bounds).
    n, N = 5, 32
    intervals = [(0, 0), (3, 9), (31, 31), (0, 31), (30, 31)]
    g = gate(n, intervals)
    assert g.num_unique_offsets() == 6
    for r_in in (0, 13, 31):
        r_out, z_0 = [1, 30, 7, 0, 31], [9, 8, 7, 6, 5]
        keys = g.gen(r_in, r_out, 41, 42, z_0)
        model = MM.gen(n, intervals, r_in, r_out, 41, 42, z_0)
        xs = list(range(N))                       # masked inputs: every group element
        got = [run_batch(g, [k] * N, xs) for k in keys]
        for party in (0, 1):
            cache = {}
            want = [MM.evaluate(n, intervals, model[party], x, cache) for x in xs]
            assert got[party] == want, (r_in, party)
        for x in xs:
            assert MM.reconstruct(n, got[0][x], got[1][x], r_out) == \
                MM.contains(intervals, (x - r_in) % N), (r_in, x)


def test_n1_all_intervals_both_inputs():
    n, N = 1, 2
    intervals = [(0, 0), (1, 1), (0, 1)]
    g = gate(n, intervals)
    for r_in in (0, 1):
        r_out, z_0 = [1, 0, 1], [0, 1, 1]
        keys = g.gen(r_in, r_out, 5, 6, z_0)
        model = MM.gen(n, intervals, r_in, r_out, 5, 6, z_0)
        got = [run_batch(g, [k, k], [0, 1]) for k in keys]
        for party in (0, 1):
            assert got[party] == [MM.evaluate(n, intervals, model[party], x) for x in (0, 1)]
        for x in (0, 1):
            assert MM.reconstruct(n, got[0][x], got[1][x], r_out) == \
                MM.contains(intervals, (x - r_in) % N)


def test_reference_small_group_case():
    # test.cc:37-113: n = 64, inputs 0..399; 12 of them against the model.
    n, N, intervals = 64, 1 << 64, REF64
    rng = np.random.default_rng(64)
    g = gate(n, intervals)
    r_in = big(rng, N)
    r_out = [big(rng, N) for _ in intervals]
    z_0 = [big(rng, N) for _ in intervals]
    keys = g.gen(r_in, r_out, 71, 72, z_0)
    model = MM.gen(n, intervals, r_in, r_out, 71, 72, z_0)
    xs = [(i + r_in) % N for i in range(400)]
    got = [run_batch(g, [k] * 400, xs) for k in keys]
    for i in range(400):
        assert MM.reconstruct(n, got[0][i], got[1][i], r_out) == MM.contains(intervals, i), i
    for j, i in enumerate((0, 9, 10, 15, 16, 30, 45, 46, 100, 250, 251, 399)):
        party = j % 2
        assert got[party][i] == MM.evaluate(n, intervals, model[party], xs[i]), i


def test_reference_large_group_case():
    # test.cc:115-208: n = 127, the ten inputs around the bounds, all bit-exact.
    n, N, intervals = 127, 1 << 127, REF127
    rng = np.random.default_rng(127)
    g = gate(n, intervals)
    r_in = big(rng, N)
    r_out = [big(rng, N) for _ in intervals]
    z_0 = [big(rng, N) for _ in intervals]
    keys = g.gen(r_in, r_out, 81, 82, z_0)
    model = MM.gen(n, intervals, r_in, r_out, 81, 82, z_0)
    plain = [2**126 - 1, 2**126, 2**126 + 1, 2**126 + 2, 2**126 + 3, 2**126 + 4,
             2**127 - 4, 2**127 - 3, 2**127 - 2, 2**127 - 1]
    xs = [(x + r_in) % N for x in plain]
    got = [run_batch(g, [k] * len(xs), xs) for k in keys]
    for party in (0, 1):
        assert got[party] == [MM.evaluate(n, intervals, model[party], x) for x in xs]
    for i, x in enumerate(plain):
        assert MM.reconstruct(n, got[0][i], got[1][i], r_out) == MM.contains(intervals, x)


def test_batch_ragged_tail_gates_straddle_waves():
    # 37 gates x 5 non-adjacent intervals: |U| = 10, 370 walks in 6 waves.
    n = 32
    c = Case(n, MM.disjoint(n, 5, np.random.default_rng(2)), 37, seed=37)
    assert c.g.num_unique_offsets() == 10
    c.check(model_gates=(0, 6, 7, 36))


def test_batch_wave_uniform_key_form():
    # 3 gates x 64-way partition: |U| = 64, every wave walks one gate's key.
    n = 32
    c = Case(n, MM.partition(n, 64), 3, seed=64)
    assert c.g.num_unique_offsets() == 64
    a, _ = c.check(model_gates=())
    for i in range(3):
        assert a[i] == c.model_row(i, i % 2)


def test_batch_one_gate_one_interval():
    c = Case(20, [(17, 900)], 1, seed=1)
    c.check(model_gates=(0,))


def test_batch_of_zero_gates_launches_nothing():
    import torch
    g = gate(32, MM.partition(32, 8))
    dev = g.upload_key_batch(g.make_key_batch([]))
    out = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
    dx = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    assert g.eval_batch_to_device(dev, dx, out) == 0
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    assert g.eval_batch([], []) == []


def test_gate_without_intervals_returns_empty():
    import torch
    g = gate(16, [])
    k0, k1 = g.gen(5, [])
    assert len(k0.output_mask_share) == 0
    assert g.eval(k0, 7) == [] and g.eval(k1, 7) == []
    dev = g.upload_key_batch(g.make_key_batch([k0, k1, k0]))
    out = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
    dx = torch.zeros((3, 2), dtype=torch.int64, device="cuda")
    assert g.eval_batch_to_device(dev, dx, out) == 0
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())


def test_full_launch_equals_the_dcf_route():
    """4096 gates x 8 non-adjacent intervals at n = 32: 65536 walks, above
    num_cus x 64 -- every CU has work, but the walks stay on the grid-stride
    loop (chunks are handed out from 2^20 walks on 256 CUs;
    test_dynamic_chunks_gpu.py covers those).  Every output equals the one
    composed from DistributedComparisonFunction.evaluate_batch_to_device on the
    2 m points per key (prepared and combined in numpy); 20 sampled gates match
    the model."""
    import torch
    from distributed_point_functions_amd import hip_abi as H
    n, N, m, gates = 32, 1 << 32, 8, 4096
    c = Case(n, MM.disjoint(n, m, np.random.default_rng(8)), gates, seed=4096)
    assert c.g.num_unique_offsets() == 2 * m
    keys = c.keys(0)
    got = np.array(run_batch(c.g, keys, c.masked), dtype=np.uint64)          # values < 2^32
    assert H.last_dynamic_chunks() == 0

    p = pb.DcfParameters()
    p.parameters.log_domain_size = n
    p.parameters.value_type.integer.bitsize = 128
    dcf = C.DistributedComparisonFunction.create(p)
    dev = dcf.upload_key_batch(dcf.make_key_batch([k.dcfkey for k in keys]))
    lo = np.array([a for a, _ in c.intervals], np.uint64)
    qp = np.array([(b + 1) % N for _, b in c.intervals], np.uint64)
    x = np.array(c.masked, np.uint64)[:, None]
    mask = np.uint64(N - 1)
    pts = np.concatenate([(x + mask - lo) & mask, (x + mask - qp) & mask], axis=1)   # [gate][2m]
    blocks = np.zeros((gates * 2 * m, 2), np.uint64)
    blocks[:, 0] = pts.reshape(-1)
    out = torch.empty(gates * 2 * m * 16, dtype=torch.uint8, device="cuda")
    dpts = torch.from_numpy(blocks.view(np.int64)).cuda()
    assert dcf.evaluate_batch_to_device(dev, dpts, 2 * m, out) == gates * 2 * m
    torch.cuda.synchronize()
    vals = out.cpu().numpy().view(np.uint64).reshape(gates, 2 * m, 2)[:, :, 0]   # mod 2^64
    party = np.array([k.dcfkey.key.party for k in keys], np.uint64)[:, None]
    z = np.array([[D.u128_from_block(s.value_uint128) for s in k.output_mask_share] for k in keys],
                 np.uint64)
    cmp_term = party * ((x > lo).astype(np.uint64) - (x > qp).astype(np.uint64))
    want = (cmp_term - vals[:, :m] + vals[:, m:] + z) & mask
    np.testing.assert_array_equal(got, want)

    rng = np.random.default_rng(20)
    for i in [0, gates - 1] + [int(v) for v in rng.integers(0, gates, size=18)]:
        assert [int(v) for v in got[i]] == c.model_row(i, i % 2), f"gate {i}"


def test_single_gate_eval_equals_the_batch_row():
    c = Case(64, REF64, 5, seed=5)
    a, b = c.check(model_gates=())
    for i in range(5):
        assert c.g.eval(c.pairs[i][i % 2], c.masked[i]) == a[i]
        assert c.g.eval(c.pairs[i][(i + 1) % 2], c.masked[i]) == b[i]
    assert c.g.eval_batch(c.keys(0), c.masked) == a


def test_errors():
    import torch
    g = gate(64, [(10, 45)])
    k0, _ = g.gen(3, [4])
    message = "Masked input should be between 0 and 2\\^log_group_size"
    with pytest.raises(D.DpfStatusError, match=message):      # test.cc:484-539
        g.eval(k0, 1 << 72)
    dev = g.upload_key_batch(g.make_key_batch([k0, k0, k0]))
    out = torch.zeros(3 * 16, dtype=torch.uint8, device="cuda")
    dx = torch.from_numpy(MM.u128_rows([1, 1 << 64, 2]).view(np.int64)).cuda()
    with pytest.raises(D.DpfStatusError, match=message) as e:
        g.eval_batch_to_device(dev, dx, out)
    assert e.value.code == 3
    dx = torch.from_numpy(MM.u128_rows([1, 2, 3]).view(np.int64)).cuda()
    with pytest.raises(D.DpfStatusError, match="device output buffer too small") as e:
        g.eval_batch_to_device(dev, dx, out[:47])
    assert e.value.code == 3
    assert g.eval_batch_to_device(dev, dx, out) == 3
    # A batch made by another gate: other interval count, other group.
    for other in (gate(64, [(10, 45), (50, 60)]), gate(32, [(10, 45)])):
        ko, _ = other.gen(3, [4] * other.num_intervals())
        odev = other.upload_key_batch(other.make_key_batch([ko, ko, ko]))
        with pytest.raises(D.DpfStatusError, match="does not match") as e:
            g.eval_batch_to_device(odev, dx, out)
        assert e.value.code == 3
