"""Per-key linear sketches of batched EvaluateUntil outputs on an MI355X
(DESIGN.md 6c): dpf_hip_sketch_rows and EvaluateUntilBatchSketchToDevice
against the Python-int model of tests/sketch_model.py over the CPU oracle's
outputs.  Exact integer arithmetic: every comparison is an equality."""
import numpy as np
import pytest

import oracle as O
import ref_grids as G
import sketch_model as M
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import heavy_hitters as HH
from test_batch_context_gpu import CASES, _check_export, _prefix_plan
from test_key_batch_gpu import _setup

pytestmark = pytest.mark.gpu

M32 = G.M32
assert M32 == (1 << 32) - 5
HH_VT = ("tuple", [("intmodn", 32, M32)] * 2)
ROW_TYPES = [
    ("intmodn", 32, M32),
    ("tuple", [("intmodn", 32, M32)] * 2),
    ("tuple", [("intmodn", 32, 1000003)] * 2),
    ("intmodn", 32, 251),
    ("tuple", [("intmodn", 32, M32)] * 5),
]
# The heavy-hitters-shaped and Mod32 cases of test_batch_context_gpu.CASES.
SKETCH_CASES = [c for c in CASES
                if all(all(kind == O.LEAF_INTMODN and bits == 32 for kind, bits, _ in O.leaves(vt))
                       for _, vt, _ in c[0])]
assert len(SKETCH_CASES) == 4


def _weights(rng, J, n, N):
    """J rows of n 32-bit weights with 0, N - 1, N and 2^32 - 1 among them."""
    w = rng.integers(0, 1 << 32, size=(J, n), dtype=np.uint64)
    special = [0, N - 1, N, (1 << 32) - 1]
    for j in range(J):
        for i in range(min(n, 4)):
            w[j, i] = special[(i + j) % 4]
    return w.astype(np.uint32)


def _dev_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


@pytest.mark.parametrize("vt", ROW_TYPES, ids=lambda v: str(v)[:40])
@pytest.mark.parametrize("K", [1, 70])
@pytest.mark.parametrize("J", [1, 2, 4])
def test_sketch_rows_against_model(vt, K, J):
    import torch
    from distributed_point_functions_amd import hip_abi as H
    mods = M.moduli(vt)
    nl = len(mods)
    desc = H.value_desc(O.leaves(vt), False, 1, 2)
    rng = np.random.default_rng(K * 100 + J * 10 + nl)
    for row_len in (1, 4, 257, 4099):
        y = np.stack([rng.integers(0, N, size=(K, row_len), dtype=np.uint64) for N in mods],
                     axis=-1).astype(np.uint32)
        # the largest residue and 0 somewhere in every row
        y[:, 0, :] = np.array(mods, dtype=np.uint32) - 1
        y[:, row_len // 2, :] = 0 if row_len > 1 else y[:, 0, :]
        w = _weights(rng, J, row_len, mods[0])
        out = torch.full((K, J, nl), -0x54545455, dtype=torch.int32, device="cuda")  # 0xAB bytes
        H.sketch_rows(K, row_len, desc, _dev_u32(y), _dev_u32(w), out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, M.sketch(vt, y.view(np.uint8), w),
                                      err_msg=f"row_len {row_len}")


def test_sketch_rows_argument_errors():
    import torch
    from distributed_point_functions_amd import hip_abi as H
    desc = H.value_desc(O.leaves(ROW_TYPES[1]), False, 1, 2)
    y = torch.zeros(8, dtype=torch.int32, device="cuda")
    w = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    with pytest.raises(H.DpfHipError) as e:
        H.sketch_rows(1, 4, desc, y, w, weight_bits=64)
    assert e.value.code == 12
    with pytest.raises(H.DpfHipError) as e:
        H.sketch_rows(1, 1 << 32, desc, y, w)
    assert e.value.code == 3
    with pytest.raises(H.DpfHipError) as e:
        H.sketch_rows(1, 4, desc, y, torch.zeros((5, 4), dtype=torch.int32, device="cuda"))
    assert e.value.code == 3
    u64 = H.value_desc([(H.LEAF_INT, 64, 0)], True, 2, 1)
    with pytest.raises(H.DpfHipError) as e:
        H.sketch_rows(1, 4, u64, y, w)
    assert e.value.code == 12


def _sketch_run(levels, plan, n_keys, seed):
    """Every level of `plan` through the sketch call with sums; checks the
    sketches against the model of the oracle's per-key outputs, the sums
    against the oracle's group sum and the exported contexts of keys 0 and
    K - 1.  Returns the bytes of every level's (sketch, sums)."""
    import torch
    dpf, P, rng, batch, oks, _, _, _ = _setup(levels, n_keys, seed=seed, party_mix=True)
    bctx = dpf.create_batch_evaluation_context(dpf.upload_key_batch(batch))
    octx = [O.create_context(P, k) for k in oks]
    seen = []
    for i, (h, prefixes) in enumerate(_prefix_plan(P, plan, rng)):
        vt = levels[h][1]
        mods = M.moduli(vt)
        size = dpf.packed_size(h)
        n_out = dpf.output_elements(h, len(prefixes), bctx.previous_hierarchy_level)
        J = (1, 2, 4, 3)[i % 4]
        w = _weights(rng, J, n_out, mods[0])
        sums = torch.full((n_out * size,), 0xAB, dtype=torch.uint8, device="cuda")
        sk = torch.full((n_keys, J, len(mods)), -0x54545455, dtype=torch.int32, device="cuda")
        n = dpf.evaluate_until_batch_sketch_to_device(h, prefixes, bctx, _dev_u32(w), sk,
                                                      sums_out=sums)
        torch.cuda.synchronize()
        assert n == n_out and bctx.previous_hierarchy_level == h
        want = [O.evaluate_until(P, h, prefixes, c) for c in octx]
        got_sk = sk.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got_sk, M.sketch(vt, np.stack(want), w),
                                      err_msg=f"level {h}")
        acc = want[0]
        for x in want[1:]:
            acc = O.add_packed(vt, acc, x)
        got_sums = sums.cpu().numpy().reshape(n_out, size)
        np.testing.assert_array_equal(got_sums, acc, err_msg=f"level {h}")
        for k in (0, n_keys - 1):
            _check_export(dpf, bctx, batch, octx, k)
        seen.append((got_sk.tobytes(), got_sums.tobytes()))
    return seen


@pytest.mark.parametrize("levels,plan", SKETCH_CASES, ids=lambda x: str(x)[:60])
@pytest.mark.parametrize("n_keys", [1, 70])
def test_batch_sketch_against_oracle(levels, plan, n_keys, monkeypatch):
    """The default path choice, the streamed path alone (DPF_BATCH_SKETCH_FUSED=0)
    and the key-major context layout all equal the model, byte for byte."""
    seed = n_keys * 3 + len(levels)
    first = _sketch_run(levels, plan, n_keys, seed)
    monkeypatch.setenv("DPF_BATCH_SKETCH_FUSED", "0")
    assert _sketch_run(levels, plan, n_keys, seed) == first
    monkeypatch.delenv("DPF_BATCH_SKETCH_FUSED")
    monkeypatch.setenv("DPF_BATCH_KEY_MAJOR", "1")
    assert _sketch_run(levels, plan, n_keys, seed) == first


def test_fused_sketch_dispatch(monkeypatch):
    """Steady-state heavy-hitters levels without duplicate prefixes and J <= 2
    run hh_keys_sketch; a duplicated prefix, J = 4 or DPF_BATCH_SKETCH_FUSED=0
    take the streamed path.  All equal the model."""
    import torch
    from distributed_point_functions_amd import hip_abi as H
    levels = [(4, HH_VT, 64.0), (6, HH_VT, 64.0), (8, HH_VT, 64.0), (10, HH_VT, 64.0),
              (12, HH_VT, 64.0)]
    n_keys = 70
    dpf, P, rng, batch, oks, _, _, _ = _setup(levels, n_keys, seed=23)
    bctx = dpf.create_batch_evaluation_context(dpf.upload_key_batch(batch))
    octx = [O.create_context(P, k) for k in oks]
    # (prefixes, J, hook, kernel expected)
    calls = [([], 2, None, None),
             ([9, 2, 14, 5], 2, None, "hh_keys_sketch"),               # shuffled, no duplicate
             ([(9 << 2) | 1, (2 << 2) | 3, (9 << 2) | 1], 2, None, "streamed"),   # a duplicate
             ([(9 << 4) | 5, (9 << 4) | 6, (2 << 4) | 12], 4, None, "streamed"),  # J beyond 2
             ([(9 << 6) | 20, (2 << 6) | 49, (9 << 6) | 24], 1, None, "hh_keys_sketch")]
    for h, (prefixes, J, hook, kernel) in enumerate(calls):
        n_out = dpf.output_elements(h, len(prefixes), bctx.previous_hierarchy_level)
        w = _weights(rng, J, n_out, M32)
        sums = torch.full((n_out * 8,), 0xAB, dtype=torch.uint8, device="cuda")
        sk = torch.full((n_keys, J, 2), -0x54545455, dtype=torch.int32, device="cuda")
        dpf.evaluate_until_batch_sketch_to_device(h, prefixes, bctx, _dev_u32(w), sk, sums_out=sums)
        torch.cuda.synchronize()
        if kernel == "hh_keys_sketch":
            assert H.last_batch_kernel() == "hh_keys_sketch", (h, H.last_batch_kernel())
        elif kernel == "streamed":
            assert H.last_batch_kernel() == "batch_level/mod32", (h, H.last_batch_kernel())
        want = [O.evaluate_until(P, h, prefixes, c) for c in octx]
        np.testing.assert_array_equal(sk.cpu().numpy().view(np.uint32),
                                      M.sketch(HH_VT, np.stack(want), w), err_msg=f"level {h}")
        acc = want[0]
        for x in want[1:]:
            acc = O.add_packed(HH_VT, acc, x)
        np.testing.assert_array_equal(sums.cpu().numpy().reshape(n_out, 8), acc)
    # the hook turns the fused path off for the same call
    monkeypatch.setenv("DPF_BATCH_SKETCH_FUSED", "0")
    bctx.reset()
    sk = torch.zeros((n_keys, 2, 2), dtype=torch.int32, device="cuda")
    dpf.evaluate_until_batch_sketch_to_device(
        0, [], bctx, _dev_u32(_weights(rng, 2, 16, M32)), sk)
    dpf.evaluate_until_batch_sketch_to_device(
        1, [9, 2, 14, 5], bctx, _dev_u32(_weights(rng, 2, 16, M32)), sk)
    assert H.last_batch_kernel() == "batch_level/mod32"


@pytest.mark.parametrize("dynamic", ["1", "0"])
def test_fused_sketch_long_tasks_and_ragged_key_group(dynamic, monkeypatch):
    """2570 keys (40 full 64-key groups and 10 lanes), 1024 start nodes: each
    wave's task is a range of several start nodes and rotates its start within
    it.  Fused == streamed for every key, and == the oracle's model for keys
    0, 63, 64, 2559 and 2569."""
    import torch
    from distributed_point_functions_amd import hip_abi as H
    from test_host_api_cpu import leaves_value
    from test_key_batch_cpu import make
    monkeypatch.setenv("DPF_HH_DYNAMIC", dynamic)
    levels = [(10, HH_VT, 64.0), (12, HH_VT, 64.0), (14, HH_VT, 64.0)]
    K = 2570
    dpf = make(levels)
    P = O.OracleParams(levels)
    rng = np.random.default_rng(2570)
    alphas = [int(x) for x in rng.integers(0, 1 << 14, size=K)]
    seeds = rng.integers(1, 1 << 62, size=(2 * K, 2), dtype=np.uint64)
    beta = [leaves_value(HH_VT, [1, 7])] * 3
    _, b1 = dpf.generate_key_batch(alphas, beta, root_seeds=seeds, threads=4)
    dev = dpf.upload_key_batch(b1)
    prefixes = [int(x) for x in rng.permutation(1024)]
    w0, w1 = _weights(rng, 2, 1024, M32), _weights(rng, 2, 4096, M32)
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("DPF_BATCH_SKETCH_FUSED", fused)
        bctx = dpf.create_batch_evaluation_context(dev)
        sums = torch.empty(4096 * 8, dtype=torch.uint8, device="cuda")
        sk = torch.full((K, 2, 2), -0x54545455, dtype=torch.int32, device="cuda")
        dpf.evaluate_until_batch_sketch_to_device(0, [], bctx, _dev_u32(w0), sk, sums_out=sums)
        dpf.evaluate_until_batch_sketch_to_device(1, prefixes, bctx, _dev_u32(w1), sk,
                                                  sums_out=sums)
        torch.cuda.synchronize()
        assert H.last_batch_kernel() == ("hh_keys_sketch" if fused == "1" else "batch_level/mod32")
        got[fused] = (sk.cpu().numpy().view(np.uint32), sums.cpu().numpy())
    np.testing.assert_array_equal(got["1"][0], got["0"][0])
    np.testing.assert_array_equal(got["1"][1], got["0"][1])
    for k in (0, 63, 64, 2559, 2569):
        s0 = int(seeds[2 * k, 0]) | int(seeds[2 * k, 1]) << 64
        s1 = int(seeds[2 * k + 1, 0]) | int(seeds[2 * k + 1, 1]) << 64
        key = O.generate_keys(P, alphas[k], [[1, 7]] * 3, s0, s1)[1]
        c = O.create_context(P, key)
        O.evaluate_until(P, 0, [], c)
        y = O.evaluate_until(P, 1, prefixes, c)
        np.testing.assert_array_equal(got["1"][0][k], M.sketch(HH_VT, y[None], w1)[0],
                                      err_msg=f"key {k}")


def test_batch_sketch_without_sums_leaves_the_same_context():
    """sums_out=None: the sketches alone; the next level still evaluates from
    the context the call left."""
    import torch
    levels, plan = SKETCH_CASES[0]
    dpf, P, rng, batch, oks, _, _, _ = _setup(levels, 9, seed=41)
    bctx = dpf.create_batch_evaluation_context(dpf.upload_key_batch(batch))
    octx = [O.create_context(P, k) for k in oks]
    for h, prefixes in _prefix_plan(P, plan, rng)[:3]:
        vt = levels[h][1]
        n_out = dpf.output_elements(h, len(prefixes), bctx.previous_hierarchy_level)
        w = _weights(rng, 2, n_out, M32)
        sk = torch.zeros((9, 2, 2), dtype=torch.int32, device="cuda")
        assert dpf.evaluate_until_batch_sketch_to_device(h, prefixes, bctx, _dev_u32(w), sk) == n_out
        torch.cuda.synchronize()
        want = [O.evaluate_until(P, h, prefixes, c) for c in octx]
        np.testing.assert_array_equal(sk.cpu().numpy().view(np.uint32),
                                      M.sketch(vt, np.stack(want), w))
        _check_export(dpf, bctx, batch, octx, 8)


def test_two_party_sketches_recombine():
    """Generated key pairs: the parties' sketches add up mod N to
    w[j][i*] * beta_e where output i* lies on alpha's path, and to 0 for a key
    whose alpha has no output at the level (its prefix was left out)."""
    import torch
    levels = [(6, HH_VT, 64.0), (8, HH_VT, 64.0), (10, HH_VT, 64.0)]
    n_keys = 12
    dpf, P, rng, _, _, alphas, _, (b0, b1) = _setup(levels, n_keys, seed=77)
    betas = [(7 * h + 3) % 200 + 1 for h in range(len(levels))]   # _setup's beta leaves
    ctxs = [dpf.create_batch_evaluation_context(dpf.upload_key_batch(b)) for b in (b0, b1)]
    prefixes = []
    left_out = 0
    for h, (log, vt, _) in enumerate(levels):
        n_out = dpf.output_elements(h, len(prefixes), ctxs[0].previous_hierarchy_level)
        w = HH.sketch_weights(5, h, n_out).astype(np.uint32)
        dw = _dev_u32(w)
        sks = []
        for c in ctxs:
            sk = torch.zeros((n_keys, 2, 2), dtype=torch.int32, device="cuda")
            assert dpf.evaluate_until_batch_sketch_to_device(h, prefixes, c, dw, sk) == n_out
            torch.cuda.synchronize()
            sks.append(sk.cpu().numpy().view(np.uint32).astype(np.uint64))
        z = (sks[0] + sks[1]) % np.uint64(M32)
        step = log - (levels[h - 1][0] if h else 0)
        vals = HH.output_values(prefixes, step, n_out)
        assert len(set(vals)) == len(vals)
        for k in range(n_keys):
            a = alphas[k] >> (levels[-1][0] - log)
            for j in range(2):
                for e in range(2):
                    want = int(w[j][vals.index(a)]) * betas[h] % M32 if a in vals else 0
                    assert int(z[k, j, e]) == want, (h, k, j, e)
            left_out += a not in vals
        # the next level's prefixes: those of the even keys only
        prefixes = sorted({alphas[k] >> (levels[-1][0] - log) for k in range(0, n_keys, 2)})
    assert left_out > 0


def test_batch_sketch_errors_leave_the_context_alone():
    import torch
    levels = [(4, HH_VT, 64.0), (6, HH_VT, 64.0), (8, HH_VT, 64.0)]
    dpf, P, rng, batch, oks, _, _, _ = _setup(levels, 4, seed=13)
    bctx = dpf.create_batch_evaluation_context(dpf.upload_key_batch(batch))
    sums = torch.empty(1 << 12, dtype=torch.uint8, device="cuda")
    sk = torch.zeros((4, 4, 2), dtype=torch.int32, device="cuda")
    w16 = torch.zeros((2, 16), dtype=torch.int32, device="cuda")
    call = dpf.evaluate_until_batch_sketch_to_device

    def fails(match, h, prefixes, w, sketch, sums_out=sums):
        before = bctx.previous_hierarchy_level
        with pytest.raises(D.DpfStatusError, match=match):
            call(h, prefixes, bctx, w, sketch, sums_out=sums_out)
        assert bctx.previous_hierarchy_level == before

    # the errors of EvaluateUntilBatch* come first
    fails("must be empty if and only if", 1, [1], torch.zeros((9, 16), dtype=torch.int32,
                                                              device="cuda"), sk)
    fails("device output buffer too small", 0, [], w16, sk, sums_out=sums[:10])
    fails(r"num_weight_rows must be in \[1, 4\]", 0, [],
          torch.zeros((5, 16), dtype=torch.int32, device="cuda"), sk)
    fails("weights_per_row does not match the number of outputs", 0, [],
          torch.zeros((2, 15), dtype=torch.int32, device="cuda"), sk)
    fails("device sketch buffer too small", 0, [], w16, sk.reshape(-1)[:15])
    assert call(0, [], bctx, w16, sk, sums_out=sums) == 16
    fails("must be greater than", 0, [1], w16, sk)
    fails("weights_per_row does not match the number of outputs", 1, [3, 5], w16, sk)
    assert call(1, [3, 5], bctx, torch.zeros((2, 8), dtype=torch.int32, device="cuda"), sk) == 8
    fails("Prefix not present in ctx.partial_evaluations at hierarchy level 1", 2, [60],
          torch.zeros((2, 4), dtype=torch.int32, device="cuda"), sk)


def test_batch_sketch_uint64_is_unimplemented():
    import torch
    levels = [(4, ("int", 64), 0), (8, ("int", 64), 0)]
    dpf, P, rng, batch, oks, _, _, _ = _setup(levels, 3, seed=17)
    bctx = dpf.create_batch_evaluation_context(dpf.upload_key_batch(batch))
    sk = torch.zeros((3, 2, 1), dtype=torch.int32, device="cuda")
    w = torch.zeros((2, 16), dtype=torch.int32, device="cuda")
    with pytest.raises(D.DpfStatusError, match="UNIMPLEMENTED.*value type not supported by the "
                                               "batched sketch"):
        dpf.evaluate_until_batch_sketch_to_device(0, [], bctx, w, sk)
    assert bctx.previous_hierarchy_level == -1


# ---------------------------------------------------------------------------
# End to end: 300 clients, two of them malformed.
# ---------------------------------------------------------------------------
E2E_LOGS = HH.hierarchy(8, 2, 24)
E2E_CLIENTS = 300
E2E_SEED = 2024
BAD_BETA, BAD_ALPHA = 5, 9


def _e2e_keys(dpf):
    """Per-client serialized keys of both parties, assembled into the two
    servers' batches: client 5 generated with beta = (2, 14), client 9's
    party-1 key taken from a key pair for a different alpha."""
    values, idx, alphas = HH.client_values(E2E_CLIENTS, seed=31, distinct=40)
    values[:, 1] = 0
    values[:, 0] &= np.uint64((1 << E2E_LOGS[-1]) - 1)
    alphas = [int(values[i, 0]) for i in idx]
    vt = HH.value_type()
    beta = [D.to_value(vt, HH.BETA)] * len(E2E_LOGS)
    seeds = np.random.default_rng(E2E_SEED).integers(0, 2**64, size=(2 * E2E_CLIENTS + 4, 2),
                                                      dtype=np.uint64)
    b0, b1 = dpf.generate_key_batch(alphas, beta, root_seeds=seeds[:2 * E2E_CLIENTS], threads=4)
    ser = [dpf.serialize_key_batch(b0), dpf.serialize_key_batch(b1)]
    bad0, bad1 = dpf.generate_key_batch([alphas[BAD_BETA]], [D.to_value(vt, (2, 14))] * len(E2E_LOGS),
                                        root_seeds=seeds[-4:-2])
    ser[0][BAD_BETA] = dpf.serialize_key_batch(bad0)[0]
    ser[1][BAD_BETA] = dpf.serialize_key_batch(bad1)[0]
    other = alphas[BAD_ALPHA] ^ (1 << (E2E_LOGS[-1] - 1))   # differs in the top bit
    _, o1 = dpf.generate_key_batch([other], beta, root_seeds=seeds[-2:])
    ser[1][BAD_ALPHA] = dpf.serialize_key_batch(o1)[0]
    return values, idx, alphas, ser


def test_heavy_hitters_flags_malformed_clients():
    import torch
    dpf = HH.create_dpf(E2E_LOGS)
    values, idx, alphas, ser = _e2e_keys(dpf)
    dev = torch.device("cuda")
    batches = [dpf.parse_key_batch(s) for s in ser]
    servers = [HH.Server(dpf, dpf.upload_key_batch(b), 4096, dev) for b in batches]
    rec, flagged = [], []
    HH.run(dpf, servers, E2E_LOGS, top_k=1024, record=rec, sketch_seed=E2E_SEED, flagged=flagged)
    assert [h for h, _ in flagged] == list(range(len(E2E_LOGS)))
    assert flagged[0][1] == [BAD_BETA, BAD_ALPHA]
    for _, bad in flagged:
        assert set(bad) <= {BAD_BETA, BAD_ALPHA}      # never an honest client
    # The caller's exclusion step: the two rejected clients' keys as their own
    # small batches at the same prefixes, subtracted from the sums.
    bad = [BAD_BETA, BAD_ALPHA]
    small = [HH.Server(dpf, dpf.upload_key_batch(dpf.parse_key_batch([s[k] for k in bad])), 4096,
                       dev) for s in ser]
    N = np.uint64(HH.MODULUS)
    keep = np.ones(E2E_CLIENTS, dtype=bool)
    keep[bad] = False
    kept_idx = idx[keep]
    prefixes = []
    for h, vals, counts, tags in rec:
        sub = np.zeros((len(vals), 2), dtype=np.uint64)
        for srv in small:
            n = srv.evaluate(h, prefixes)
            assert n == len(vals)
            sub = (sub + srv.out[: n * 8].cpu().numpy().view(np.uint32).reshape(-1, 2)) % N
        c = (counts.astype(np.uint64) + N - sub[:, 0]) % N
        t = (tags.astype(np.uint64) + N - sub[:, 1]) % N
        HH.verify([(h, vals, c, t)], E2E_LOGS, values, kept_idx)
        prefixes = HH.select(vals, counts, 1024)
