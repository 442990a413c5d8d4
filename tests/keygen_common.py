"""Helpers shared by the batched key generation tests (test_keygen_cpu.py,
test_keygen_gpu.py): key batches as numpy arrays, and the batch the CPU oracle's
single-key generation gives for the same alphas, betas and root seeds."""
import numpy as np

import oracle as O

MASK64 = (1 << 64) - 1


def seed_ints(seeds, k):
    s0 = int(seeds[2 * k, 0]) | int(seeds[2 * k, 1]) << 64
    s1 = int(seeds[2 * k + 1, 0]) | int(seeds[2 * k + 1, 1]) << 64
    return s0, s1


def batch_arrays(b):
    """Every array of a host KeyBatch."""
    return {"seed": b.seeds(), "party": b.party(), "cw_seed": b.cw_seeds(),
            "cw_left": b.cw_left(), "cw_right": b.cw_right(),
            **{f"vc{h}": b.value_correction(h) for h in range(b.num_hierarchy_levels)}}


def assert_batches_equal(got, want, what=""):
    g, w = batch_arrays(got), batch_arrays(want)
    assert g.keys() == w.keys(), what
    assert got.num_keys == want.num_keys and got.num_levels == want.num_levels, what
    for name in w:
        np.testing.assert_array_equal(g[name], w[name], err_msg=f"{what} {name}")


def oracle_arrays(P, okeys):
    """The arrays of the batch holding the oracle's keys `okeys` (one party)."""
    H = len(P.log_domain)
    L = P.tree_levels_needed - 1
    n = len(okeys)
    out = {"seed": O.blocks_from_ints([k["seed"] for k in okeys]).reshape(n, 2),
           "party": np.array([k["party"] for k in okeys], np.uint8)}
    cws, cl, cr = [], [], []
    for k in okeys:
        cws += [c[0] for c in k["cws"][:L]]
        cl += [c[1] for c in k["cws"][:L]]
        cr += [c[2] for c in k["cws"][:L]]
    out["cw_seed"] = (O.blocks_from_ints(cws) if cws else np.zeros((0, 2), np.uint64)).reshape(-1, 2)
    out["cw_left"] = np.array(cl, np.uint8)
    out["cw_right"] = np.array(cr, np.uint8)
    for h in range(H):
        flat = [x for k in okeys for elem in O._value_correction(P, k, h) for x in elem]
        out[f"vc{h}"] = O.blocks_from_ints(flat).reshape(-1, 2)
    return out


def assert_batch_equals_oracle(got, P, okeys, what=""):
    g, w = batch_arrays(got), oracle_arrays(P, okeys)
    assert g.keys() == w.keys(), what
    for name in w:
        np.testing.assert_array_equal(g[name], w[name], err_msg=f"{what} {name}")
