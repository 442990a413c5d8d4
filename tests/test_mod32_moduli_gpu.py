"""Every copy of the mod-N sampling loop and every user of mul_mod, mod32 and
mod64 on an MI355X, at moduli that take BOTH corrections of div_2by1
(csrc/kernels/dpf_device.h) both ways.

2^32 - 5, the modulus of nearly every other test, always takes the first
correction and never the second: a kernel that lost the second correction, or
applied the first unconditionally, passes every test at that modulus.  The
grid of tests/div32_cases.py adds 0x80010001, 65537 and 17 (which reach the
second correction at shifts 0, 15 and 27) and 2^31; that every case below
reaches the branches it is there for is proved on the CPU, from the oracle and
the model alone, by tests/test_div32_model_cpu.py.

Every comparison is an equality against the CPU oracle or Python-integer
arithmetic; the kernel that ran is read from the dispatch reporters.
"""
import numpy as np
import pytest

import div32_cases as C
import oracle as O
import sketch_model as SM
import test_batch_context_gpu as TB
import test_full_domain_sketch_gpu as TF
import test_kernels_gpu as TK
from distributed_point_functions_amd import hip_abi
from test_host_api_cpu import leaves_value
from test_key_batch_cpu import make
from test_key_batch_gpu import _setup

pytestmark = pytest.mark.gpu

POISON = -0x54545455     # 0xAB bytes


@pytest.fixture(scope="module")
def hip():
    import torch
    hip_abi.load(require_gpu=True)
    assert torch.cuda.is_available()
    return hip_abi


def _dev_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


# ---- 1. full-domain expansion: small, pair and octet kernels --------------------------------
@pytest.mark.parametrize("nl", C.EXPAND_LEAVES)
@pytest.mark.parametrize("N", C.GRID, ids=hex)
@pytest.mark.parametrize("shape", C.EXPAND_SHAPES, ids=str)
def test_expand_every_modulus(hip, shape, N, nl, monkeypatch):
    """IntModN<N>, Tuple<IntModN<N> x2> and x5 of both parties through the
    small-tree, pair and octet kernels (Mod32Leaf<2> and <5>); value
    corrections N - 1, 0, 1 and random.  Each shape runs as dispatched and
    under the hooks that send it to the pair kernel (div32_cases.expand_runs).
    One modulus runs at security 40 and 64."""
    levels, n0 = C.EXPAND_SHAPES[shape]
    vt = C.value_type(N, nl)
    for sec in (40.0, 64.0) if N == C.EXPAND_SEC64 else (40.0,):
        for party in (0, 1):
            inputs = C.expand_inputs(shape, N, nl, party)
            for hooks, want in C.expand_runs(shape, nl):
                for name, value in hooks.items():
                    monkeypatch.setenv(name, value)
                TK._expand_case(hip, None, vt, n0, levels, party, sec=sec, inputs=inputs)
                assert hip.last_expand_kernel()[0] == want, (sec, party, hooks)
                for name in hooks:
                    monkeypatch.delenv(name)


# ---- 2. batched prefix evaluation: hh_keys, hh_level, batch_level/mod32 ---------------------
@pytest.mark.parametrize("nl", C.BATCH_LEAVES)
@pytest.mark.parametrize("N", C.BATCH_MODULI, ids=hex)
def test_batch_levels_every_kernel(N, nl, monkeypatch):
    """A heavy-hitters-shaped hierarchy per key (70 keys: the general kernel's
    mod32 leaf) and summed over 130 keys: hh_keys by default, hh_level with the
    key-major tables, the general kernel with DPF_BATCH_NO_LEAN=1.  Outputs
    and exported contexts against the oracle (test_batch_context_gpu._run)."""
    levels, plan = C.batch_levels(N, nl)
    seen = {}
    TB._run(levels, plan, C.BATCH_KEYS[False], False, seed=C.batch_seed(N, nl, C.BATCH_KEYS[False]))
    seen["per key"] = hip_abi.last_batch_kernel()
    k = C.BATCH_KEYS[True]
    for name, hook in (("sum", None), ("key major", "DPF_BATCH_KEY_MAJOR"),
                       ("no lean", "DPF_BATCH_NO_LEAN")):
        if hook:
            monkeypatch.setenv(hook, "1")
        TB._run(levels, plan, k, True, seed=C.batch_seed(N, nl, k))
        seen[name] = hip_abi.last_batch_kernel()
        if hook:
            monkeypatch.delenv(hook)
    assert seen == {"per key": "batch_level/mod32", "sum": "hh_keys", "key major": "hh_level",
                    "no lean": "batch_level/mod32"}


@pytest.mark.parametrize("nl", C.BATCH_LEAVES)
@pytest.mark.parametrize("N", C.BATCH_MODULI, ids=hex)
def test_fused_sketch_every_level(N, nl, monkeypatch):
    """hh_keys_sketch (sample2 and mul_mod in one kernel, sketch_finish's mod64,
    sketch_slot_weights' mod32) on every cached level, against sketch_model
    over the oracle's per-key outputs and the oracle's group sum; the streamed
    path (DPF_BATCH_SKETCH_FUSED=0) gives the same bytes."""
    import torch
    levels, _ = C.batch_levels(N, nl)
    vt = levels[0][1]
    n_keys = C.FUSED_KEYS
    size = 4 * nl
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("DPF_BATCH_SKETCH_FUSED", fused)
        dpf, P, rng, batch, oks, _, _, _ = _setup(levels, n_keys, seed=C.fused_seed(N, nl))
        bctx = dpf.create_batch_evaluation_context(dpf.upload_key_batch(batch))
        octx = [O.create_context(P, k) for k in oks]
        got[fused] = []
        for h, prefixes in C.FUSED_CALLS:
            n_out = dpf.output_elements(h, len(prefixes), bctx.previous_hierarchy_level)
            w = C.weights(rng, 2, n_out, N)
            sums = torch.full((n_out * size,), 0xAB, dtype=torch.uint8, device="cuda")
            sk = torch.full((n_keys, 2, nl), POISON, dtype=torch.int32, device="cuda")
            assert dpf.evaluate_until_batch_sketch_to_device(h, prefixes, bctx, _dev_u32(w), sk,
                                                             sums_out=sums) == n_out
            torch.cuda.synchronize()
            if h > 0:
                assert hip_abi.last_batch_kernel() == (
                    "hh_keys_sketch" if fused == "1" else "batch_level/mod32"), (h, fused)
            want = [O.evaluate_until(P, h, prefixes, c) for c in octx]
            got_sk = sk.cpu().numpy().view(np.uint32)
            np.testing.assert_array_equal(got_sk, SM.sketch(vt, np.stack(want), w),
                                          err_msg=f"level {h} fused {fused}")
            acc = want[0]
            for x in want[1:]:
                acc = O.add_packed(vt, acc, x)
            got_sums = sums.cpu().numpy().reshape(n_out, size)
            np.testing.assert_array_equal(got_sums, acc, err_msg=f"level {h} fused {fused}")
            got[fused].append((got_sk.tobytes(), got_sums.tobytes()))
    assert got["1"] == got["0"]


# ---- 3. dpf_hip_sketch_rows: mod32, mul_mod with unreduced rows, mod64 ----------------------
@pytest.mark.parametrize("N", C.GRID, ids=hex)
def test_sketch_rows_every_modulus(hip, N):
    """Rows that are NOT reduced (N, N + 1, 2^32 - 1 among the entries; the
    header bounds `in` by nothing and mul_mod takes any 32-bit y), weights 0,
    N - 1, N and 2^32 - 1, and directed pairs on which mul_mod takes its second
    correction, against sketch_model.sketch in Python integers."""
    import torch
    vt = C.value_type(N, C.SKETCH_NL)
    desc = hip.value_desc(O.leaves(vt), False, 1, 2)
    for K in C.SKETCH_K:
        for row_len in C.SKETCH_ROW_LEN:
            for J in C.SKETCH_J:
                y, w = C.sketch_rows_case(N, K, row_len, J)
                out = torch.full((K, J, C.SKETCH_NL), POISON, dtype=torch.int32, device="cuda")
                hip.sketch_rows(K, row_len, desc, _dev_u32(y), _dev_u32(w), out=out)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32),
                                              SM.sketch(vt, y.view(np.uint8), w),
                                              err_msg=f"K {K} row_len {row_len} J {J}")


# ---- 4. checked histograms: dpf_hip_expand_sketch -------------------------------------------
def _hist_rows(nl, n, party):
    """The oracle's full-domain rows of the case's 65 keys: uint32 [K][2^n][nl]
    and the packed bytes [K][...]."""
    P, keys = C.hist_oracle_keys(nl, n, party)
    ys = [np.ascontiguousarray(O.evaluate_until(P, 0, [], O.create_context(P, k))) for k in keys]
    packed = np.stack(ys).reshape(len(keys), -1)
    return packed.view("<u4").reshape(len(keys), 1 << n, nl).copy(), packed


@pytest.mark.parametrize("n", C.HIST_DOMAINS)
@pytest.mark.parametrize("nl", [1, 2])
def test_histogram_at_a_modulus_that_takes_both_corrections(nl, n):
    """IntModN<0x80010001> and its 2-tuple, one key and 65 keys of both
    parties, two weight rows: sums and sketches against the oracle's rows
    reduced in Python integers; the parties' sums reconstruct the histogram;
    one accumulate starts from entries N - 1."""
    vt = C.value_type(C.HIST_N, nl)
    mods = [C.HIST_N] * nl
    alphas, betas, seeds, w = C.hist_case(nl, n)
    dpf = make([(n, vt, 0)])
    assert dpf.evaluates_full_domain_sum_sketch_on_device(0)
    host = dpf.generate_key_batch_with_betas(alphas, [leaves_value(vt, b) for b in betas],
                                             root_seeds=seeds)
    dw = _dev_u32(w)
    dom = 1 << n
    shares = {}
    for party in (0, 1):
        rows, packed = _hist_rows(nl, n, party)
        for K in C.HIST_KEYS:
            dev = dpf.upload_key_batch(host[party], 0, K)
            got_sum, got_sk = TF._run(dpf, dev, 0, n, nl, dw)
            want_sum = TF._mod_sum(rows[:K], mods)
            np.testing.assert_array_equal(got_sum, want_sum, err_msg=f"party {party} K {K}")
            np.testing.assert_array_equal(got_sk, SM.sketch(vt, packed[:K], w),
                                          err_msg=f"party {party} K {K}")
            shares[party, K] = want_sum
        # 65 keys onto a buffer of N - 1 everywhere: every modular add wraps
        # or lands on N - 1 exactly.
        top = np.full((dom, nl), C.HIST_N - 1, dtype=np.uint32)
        got, sk = TF._run(dpf, dev, 0, n, nl, dw, accumulate=True, out=_dev_u32(top).clone())
        np.testing.assert_array_equal(got, TF._mod_sum([top, shares[party, 65]], mods))
        np.testing.assert_array_equal(sk, SM.sketch(vt, packed, w))
    hist = np.zeros((dom, nl), dtype=object)
    for a, b in zip(alphas, betas):
        hist[a] += np.array(b, dtype=object)
    hist = (hist % C.HIST_N).astype(np.uint32)
    np.testing.assert_array_equal(TF.HG.reconstruct_mod(shares[0, 65], shares[1, 65], mods), hist)


@pytest.mark.parametrize("mods", C.ABI_PAIRS, ids=str)
def test_two_moduli_that_take_both_corrections_at_the_c_abi(mods):
    """(0x80010001, 65537) and the reverse: shift 0 next to shift 15 in one
    tuple, both reaching the second correction; a leaf or modulus index mix-up
    between the two Div32 of the kernel shows.  The model of
    test_full_domain_sketch_gpu (oracle tree and value hash, sampled in Python
    integers) is the reference."""
    import torch
    n, K = C.ABI_N, C.ABI_KEYS
    keys, corrs, w = C.abi_case(mods)
    rows = [TF._model_rows(key, n, mods, corr, k & 1)
            for k, (key, corr) in enumerate(zip(keys, corrs))]
    desc = hip_abi.value_desc([(hip_abi.LEAF_INTMODN, 32, m) for m in mods], False, 1, 2)
    cw = [O._cw_arrays(key, 0, n) for key in keys]
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
    np.testing.assert_array_equal(got_sum.cpu().numpy().view(np.uint32), TF._mod_sum(rows, mods))
    want_sk = np.zeros((K, 2, 2), dtype=np.uint32)
    for e, m in enumerate(mods):
        y = np.stack(rows)[:, :, e].astype(object)
        want_sk[:, :, e] = (np.dot(w.astype(object) % m, y.T) % m).T.astype(np.uint32)
    np.testing.assert_array_equal(got_sk.cpu().numpy().view(np.uint32), want_sk)
