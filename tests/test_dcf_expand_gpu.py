"""Full-domain DCF evaluation on an MI355X (dpf_hip_dcf_expand): bit-exact
against the oracle's Evaluate on small domains, byte for byte against the
per-point kernel (itself oracle-verified, test_dcf_gpu.py) on domains large
enough for every path of the launch plan -- items that walk from the key's
root, items that visit their subtree depth-first, items started from the roots
a first launch stored -- and shards, key batches, the dynamic item loop and
the range query folded over a database."""
import numpy as np
import pytest

import oracle as O
from distributed_point_functions_amd import dpf as D
from distributed_point_functions_amd import hip_abi
from test_dcf_cpu import make
from test_host_api_cpu import leaves_value

pytestmark = pytest.mark.gpu

MASK64 = (1 << 64) - 1


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _full(dcf, key, n, shard=0, num_shards=1):
    """uint8 (2^n / num_shards, packed_size) through the device call."""
    import torch
    size = dcf.packed_size()
    rows = (1 << n) // num_shards
    out = torch.empty(rows * size, dtype=torch.uint8, device="cuda")
    assert dcf.evaluate_full_domain_to_device(key, out, shard=shard, num_shards=num_shards) == rows
    return out.cpu().numpy().reshape(rows, size)


def _all_points(n):
    xs = np.zeros((1 << n, 2), dtype=np.uint64)
    xs[:, 0] = np.arange(1 << n, dtype=np.uint64)
    return xs


def _beta(vt):
    return (1 << vt[1]) - 3 if vt[0] == "int" else 0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A >> (128 - vt[1])


@pytest.mark.parametrize("vt", [("int", 64), ("int", 8), ("int", 128), ("xor", 64)], ids=str)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_oracle_parity_both_parties(n, vt):
    dcf = make(vt, n)
    assert dcf.evaluates_full_domain_on_device()
    P = O.dcf_params(n, vt)
    beta = [_beta(vt)]
    xs = range(1 << n)
    for alpha in sorted({0, 1, 1 << (n - 1), (1 << n) - 1}):
        keys = dcf.generate_keys(alpha, leaves_value(vt, beta), seed_0=alpha + 5, seed_1=alpha + 91)
        okeys = O.dcf_generate_keys(P, alpha, beta, alpha + 5, alpha + 91)
        shares = []
        for k, ok in zip(keys, okeys):
            want = np.concatenate([O.dcf_evaluate(P, ok, x) for x in xs])
            got = dcf.evaluate_full_domain_packed(k)
            np.testing.assert_array_equal(got, want, err_msg=f"alpha={alpha} packed")
            np.testing.assert_array_equal(_full(dcf, k, n), want, err_msg=f"alpha={alpha} device")
            shares.append(got)
        if vt[0] == "int":
            total = O.unpack_elements(vt, O.add_packed(vt, shares[0], shares[1]))
            for x in xs:
                assert total[x] == (beta if x < alpha else [0]), (alpha, x)


# n = 12 and 16: every item one last-level node; 20: depth-first items that
# walk from the root; 22: depth-first items started from stored roots (on a
# 256-CU device; the plan's properties are pinned in test_dcf_expand_cpu.py).
@pytest.mark.parametrize("vt", [("int", 16), ("int", 32), ("int", 64), ("xor", 128)], ids=str)
@pytest.mark.parametrize("n", [12, 16, 20, 22])
def test_parity_with_the_per_point_kernel(n, vt):
    dcf = make(vt, n)
    pl = hip_abi.dcf_expand_plan(1, n, 0, _cus())
    k = pl["walk"]
    G = pl["G"]
    xs = _all_points(n)
    # Subtree boundaries and just off them: the walk depth's power of two,
    # and the last item's first output less one.
    alphas = [(1 << k) - 1, 1 << k, (1 << k) + 1, (1 << n) - (1 << (G + 1)) - 1]
    alphas = sorted({a for a in alphas if 0 <= a < (1 << n)})
    for i, alpha in enumerate(alphas):
        key = dcf.generate_keys(alpha, leaves_value(vt, [_beta(vt)]), seed_0=n + i, seed_1=77 + i)[i % 2]
        want = dcf.evaluate_packed(key, xs)
        np.testing.assert_array_equal(_full(dcf, key, n), want, err_msg=f"alpha={alpha} {pl}")


def test_the_plan_takes_every_path_on_this_device():
    cus = _cus()
    assert hip_abi.dcf_expand_plan(1, 12, 0, cus)["G"] == 0
    p20, p22 = hip_abi.dcf_expand_plan(1, 20, 0, cus), hip_abi.dcf_expand_plan(1, 22, 0, cus)
    assert p20["G"] > 0 and p20["top_G"] == -1
    assert p22["top_G"] >= 0


@pytest.mark.parametrize("n,num_shards", [(10, 1), (10, 2), (10, 512), (22, 4)])
def test_shards_are_slices(n, num_shards):
    vt = ("int", 64)
    dcf = make(vt, n)
    alpha = (3 << (n - 2)) + 5
    key = dcf.generate_keys(alpha, 7, seed_0=3, seed_1=4)[1]
    whole = _full(dcf, key, n)
    rows = (1 << n) // num_shards
    for shard in sorted({0, num_shards - 1}):
        got = _full(dcf, key, n, shard, num_shards)
        np.testing.assert_array_equal(got, whole[shard * rows:(shard + 1) * rows],
                                      err_msg=f"shard {shard}")


def _batch_keys(dcf, n, nk, seed):
    rng = np.random.default_rng(seed)
    keys = []
    for k in range(nk):
        alpha = int(rng.integers(0, 1 << n))
        keys.append(dcf.generate_keys(alpha, 1000 + k, seed_0=k + 1, seed_1=k + 500)[k % 2])
    return keys


@pytest.mark.parametrize("nk", [1, 3, 37])
def test_key_batches_rows_equal_single_key_calls(nk):
    import torch
    n, vt = 9, ("int", 64)
    dcf = make(vt, n)
    keys = _batch_keys(dcf, n, nk, nk)
    dev = dcf.upload_key_batch(dcf.make_key_batch(keys))
    out = torch.empty(nk << n, dtype=torch.int64, device="cuda")
    assert dcf.evaluate_full_domain_batch_to_device(dev, out) == nk << n
    got = out.cpu().numpy().view(np.uint8).reshape(nk, 1 << n, 8)
    for k in range(nk):
        np.testing.assert_array_equal(got[k], _full(dcf, keys[k], n), err_msg=f"key {k}")
    # The last shard of four, for every key.
    out4 = torch.empty(nk << (n - 2), dtype=torch.int64, device="cuda")
    assert dcf.evaluate_full_domain_batch_to_device(dev, out4, shard=3, num_shards=4) == nk << (n - 2)
    np.testing.assert_array_equal(out4.cpu().numpy().view(np.uint8).reshape(nk, -1, 8),
                                  got[:, 3 << (n - 2):])


def test_device_generated_key_batch():
    import torch
    n, vt, nk = 9, ("int", 64), 37
    dcf = make(vt, n)
    rng = np.random.default_rng(9)
    alphas = [int(a) for a in rng.integers(0, 1 << n, size=nk)]
    seeds = rng.integers(0, 1 << 63, size=(2 * nk, 2), dtype=np.uint64)
    values = [leaves_value(vt, [11 + k]) for k in range(nk)]
    dev = dcf.generate_key_batch_to_device(alphas, values, root_seeds=seeds)
    outs = []
    for d in dev:
        out = torch.empty(nk << n, dtype=torch.int64, device="cuda")
        assert dcf.evaluate_full_domain_batch_to_device(d, out) == nk << n
        outs.append(out.cpu().numpy().view(np.uint64).reshape(nk, 1 << n))
    total = outs[0] + outs[1]
    x = np.arange(1 << n)
    for k in range(nk):
        np.testing.assert_array_equal(total[k], np.where(x < alphas[k], 11 + k, 0).astype(np.uint64))
    # Row k is the single-key call on the key the host generates from the same seeds.
    s0 = int(seeds[10, 0]) | int(seeds[10, 1]) << 64
    s1 = int(seeds[11, 0]) | int(seeds[11, 1]) << 64
    key = dcf.generate_keys(alphas[5], values[5], seed_0=s0, seed_1=s1)[0]
    np.testing.assert_array_equal(outs[0][5], _full(dcf, key, n).view(np.uint64).reshape(-1))


def test_many_keys_depth_first_with_a_one_node_top_launch():
    """1024 keys of 2^13 outputs: waves of items per key, a top launch whose
    items are single nodes -- against the per-point kernel on shared points."""
    import torch
    n, vt, nk = 13, ("int", 64), 1024
    pl = hip_abi.dcf_expand_plan(nk, n, 0, _cus())
    dcf = make(vt, n)
    keys = _batch_keys(dcf, n, nk, 13)
    dev = dcf.upload_key_batch(dcf.make_key_batch(keys))
    out = torch.empty(nk << n, dtype=torch.int64, device="cuda")
    assert dcf.evaluate_full_domain_batch_to_device(dev, out) == nk << n
    pts = torch.from_numpy(_all_points(n).view(np.int64)).cuda()
    want = torch.empty(nk << n, dtype=torch.int64, device="cuda")
    assert dcf.evaluate_batch_to_device(dev, pts, 1 << n, want, shared_points=True) == nk << n
    assert torch.equal(out, want), pl


def test_batch_of_another_dcf_is_rejected_first():
    import torch
    dcf9, dcf8 = make(("int", 64), 9), make(("int", 64), 8)
    dev = dcf8.upload_key_batch(dcf8.make_key_batch(_batch_keys(dcf8, 8, 2, 1)))
    out = torch.empty(2 << 9, dtype=torch.int64, device="cuda")
    with pytest.raises(D.DpfStatusError) as e:
        dcf9.evaluate_full_domain_batch_to_device(dev, out[:1], num_shards=3)
    assert e.value.message == "key batch does not match this DistributedComparisonFunction"
    with pytest.raises(D.DpfStatusError) as e:
        dcf8.evaluate_full_domain_batch_to_device(dev, out[:1], num_shards=3)
    assert e.value.message == "num_shards must be a power of two and 0 <= shard < num_shards"
    with pytest.raises(D.DpfStatusError) as e:
        dcf8.evaluate_full_domain_batch_to_device(dev, out[:1])
    assert e.value.message == "device output buffer too small"


def test_dynamic_and_static_item_loops_agree(monkeypatch):
    """The smallest domain of one key whose launch gives every wave four
    chunks of 64 items: the same outputs with the loop dynamic (default) and
    with DPF_DCF_EXPAND_DYNAMIC=0, each run reporting its own loop."""
    import torch
    cus = _cus()
    n = next(n for n in range(1, 40) if hip_abi.dcf_expand_plan(1, n, 0, cus)["items"] >= cus * 4096)
    assert hip_abi.dcf_expand_plan(1, n - 1, 0, cus)["items"] < cus * 4096
    vt = ("int", 8)
    dcf = make(vt, n)
    key = dcf.generate_keys((5 << (n - 3)) + 1, 3, seed_0=8, seed_1=9)[1]
    outs = []
    for hook, dynamic in ((None, True), ("0", False)):
        if hook is None:
            monkeypatch.delenv("DPF_DCF_EXPAND_DYNAMIC", raising=False)
        else:
            monkeypatch.setenv("DPF_DCF_EXPAND_DYNAMIC", hook)
        out = torch.empty(1 << n, dtype=torch.uint8, device="cuda")
        assert dcf.evaluate_full_domain_to_device(key, out) == 1 << n
        assert (hip_abi.last_dynamic_chunks() > 0) == dynamic, (n, hook)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    # Against the per-point kernel at the ends and around alpha.
    alpha = (5 << (n - 3)) + 1
    xs = [0, 1, alpha - 1, alpha, alpha + 1, (1 << n) - 2, (1 << n) - 1]
    want = dcf.evaluate_packed(key, xs).reshape(-1)
    np.testing.assert_array_equal(outs[0][torch.tensor(xs, device="cuda")].cpu().numpy(), want)


@pytest.mark.parametrize("slab_log", [None, "10"])
@pytest.mark.parametrize("w", [1, 3])
def test_range_dot_reconstructs_the_prefix_sum(w, slab_log, monkeypatch):
    import torch
    if slab_log is None:
        monkeypatch.delenv("DPF_DOT_SLAB_LOG", raising=False)
    else:
        monkeypatch.setenv("DPF_DOT_SLAB_LOG", slab_log)    # four slabs per whole-domain call
    n, vt, beta, alpha = 12, ("int", 64), 0x123456789ABCDEF1, 2741
    dcf = make(vt, n)
    keys = dcf.generate_keys(alpha, beta, seed_0=21, seed_1=22)
    rng = np.random.default_rng(w)
    db = rng.integers(0, 1 << 63, size=(1 << n, w), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    ddb = torch.from_numpy(db.view(np.int64)).cuda()
    want = (db[:alpha].sum(axis=0, dtype=np.uint64) * np.uint64(beta))
    parts = []
    for key in keys:
        f = _full(dcf, key, n).view(np.uint64).reshape(-1)
        fold = (f[:, None] * db).sum(axis=0, dtype=np.uint64)
        out = torch.zeros(w, dtype=torch.int64, device="cuda")
        assert dcf.evaluate_range_dot_to_device(key, ddb, w, out) == w
        one = out.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(one, fold)
        np.testing.assert_array_equal(dcf.evaluate_range_dot(key, ddb, w), fold)
        # Four shards, each over its own records, summed.
        rows = 1 << (n - 2)
        acc = np.zeros(w, dtype=np.uint64)
        for shard in range(4):
            out4 = torch.zeros(w, dtype=torch.int64, device="cuda")
            dcf.evaluate_range_dot_to_device(key, ddb[shard * rows:(shard + 1) * rows], w, out4,
                                             shard=shard, num_shards=4)
            acc += out4.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(acc, fold)
        parts.append(one)
    np.testing.assert_array_equal(parts[0] + parts[1], want)
