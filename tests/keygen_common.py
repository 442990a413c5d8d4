"""Helpers shared by the batched key generation tests (test_keygen_cpu.py,
test_keygen_gpu.py, the key generation section of test_dynamic_chunks_gpu.py):
key batches as numpy arrays, the batch the CPU oracle's single-key generation
gives for the same alphas, betas and root seeds, level lists at the edges of
the kernel's level tables, an arena with gaps for the output arrays of a C ABI
call, and the key pairs at the boundaries of the chunked schedule."""
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


# Level lists at the edges of the key generation kernel's level tables, with the
# hierarchy_to_tree each must give (test_keygen_cpu.py pins the host generator to
# the oracle on them, test_keygen_gpu.py the device generator to both).
_WIDTHS = [(4, 8), (7, 16), (9, 32), (10, 64), (12, 128)]   # 4, 3, 2, 1, 0 index bits
EDGE_LEVELS = [
    # The first level's prefix is alpha >> 128; the alpha bit at shift 127 is the
    # first tree step.
    ([(0, ("int", 64), 0), (128, ("int", 64), 0)], [0, 127]),
    ([(0, ("xor", 128), 0), (64, ("int", 16), 0), (128, ("xor", 8), 0)], [0, 61, 124]),
    # Every width at an inner level with a block index.
    ([(log, ("int", bits), 0) for log, bits in _WIDTHS], [0, 4, 7, 9, 12]),
    ([(log, ("xor", bits), 0) for log, bits in _WIDTHS], [0, 4, 7, 9, 12]),
    # Value corrections from consecutive tree levels.
    ([(1, ("int", 8), 0), (2, ("int", 16), 0), (3, ("xor", 32), 0), (4, ("int", 64), 0),
      (5, ("xor", 128), 0)], [0, 1, 2, 3, 5]),
    ([(3, ("int", 8), 0), (4, ("int", 8), 0), (5, ("int", 8), 0)], [0, 1, 2]),
]


def assert_arrays_equal(got, want, what=""):
    """Two dicts of key batch arrays (batch_arrays, oracle_arrays,
    KeygenArena.arrays), name by name; the root seeds and party bytes, which key
    generation does not compute, may be missing from either."""
    inputs = {"seed", "party"}
    assert got.keys() - inputs == want.keys() - inputs, (what, sorted(got), sorted(want))
    for name in sorted(got.keys() & want.keys()):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype, (what, name, g.dtype, w.dtype)
        # np.testing takes ten times as long on arrays of tens of megabytes: it
        # only writes the report.
        if not np.array_equal(g, w):
            np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")
            raise AssertionError(f"{what} {name}")


def rows_of(arrays, ks, num_keys):
    """The rows of the key pairs `ks` of a batch's arrays, as the arrays of the
    batch that holds just those keys (every array is key-major)."""
    out = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        assert a.shape[0] % num_keys == 0, name
        per = a.shape[0] // num_keys
        idx = (np.asarray(ks, np.int64)[:, None] * per + np.arange(per)[None, :]).reshape(-1)
        out[name] = a[idx]
    return out


class KeygenArena:
    """The output arrays of one dpf_hip_gen_key_batch call -- cw_seed, cw_left,
    cw_right and vc{h} of `elements[h]` blocks per key -- carved out of one
    uint8 tensor on `device` prefilled with `fill`.  Every array starts on a
    16-byte boundary plus offsets.get(name, 0) and is followed by at least
    GAP bytes nothing may write; GUARD more end the arena.  (With a guard at
    the end alone, an overrun of one array into its neighbour would be
    overwritten by the neighbour's own data.)"""
    GAP, GUARD = 64, 4096

    def __init__(self, num_keys, num_levels, elements, fill, device="cuda", offsets=None):
        import torch
        offsets = offsets or {}
        sizes = [("cw_seed", num_keys * num_levels * 16), ("cw_left", num_keys * num_levels),
                 ("cw_right", num_keys * num_levels)]
        sizes += [(f"vc{h}", num_keys * e * 16) for h, e in enumerate(elements)]
        assert set(offsets) <= {name for name, _ in sizes}
        self.fill, self.spans = fill, {}
        pos = self.GAP
        for name, nbytes in sizes:
            pos = -(-pos // 16) * 16 + offsets.get(name, 0)
            self.spans[name] = (pos, nbytes)
            pos += nbytes + self.GAP
        self.size = pos + self.GUARD
        # 16 spare bytes: the arena proper begins on a 16-byte boundary of the
        # address space, wherever the allocation does.
        self.raw = torch.full((self.size + 16,), fill, dtype=torch.uint8, device=device)
        self.base = -self.raw.data_ptr() % 16
        for name, (start, _) in self.spans.items():
            assert (self.raw.data_ptr() + self.base + start) % 16 == offsets.get(name, 0), name

    def tensor(self, name):
        """The uint8 view of one array (its data_ptr is what the call gets)."""
        start, nbytes = self.spans[name]
        return self.raw[self.base + start:self.base + start + nbytes]

    def value_corrections(self):
        return [self.tensor(f"vc{h}") for h in range(len(self.spans) - 3)]

    def arrays(self):
        """The arrays by batch_arrays' names (blocks as uint64 (n, 2), control
        bytes as uint8), once every byte outside them still holds the prefill."""
        host = self.raw.cpu().numpy()
        out, bad, end = {}, [], 0
        # The spans lie in order: what is between them is gap (or guard).
        for name, (start, nbytes) in list(self.spans.items()) + [(None, (len(host) - self.base, 0))]:
            lo = self.base + start
            gap = host[end:lo]
            bad += (end + np.flatnonzero(gap != self.fill)).tolist()
            end = lo + nbytes
            if name is not None:
                a = host[lo:end].copy()
                out[name] = a if name in ("cw_left", "cw_right") else a.view(np.uint64).reshape(-1, 2)
        if bad:
            at = bad[0] - self.base
            raise AssertionError(f"{len(bad)} bytes outside the arrays written, the first at arena "
                                 f"offset {at} ({self._where(at)})")
        return out

    def _where(self, at):
        """Which gap an arena offset lies in."""
        before = [(s + n, name) for name, (s, n) in self.spans.items() if s + n <= at]
        if not before:
            return "before cw_seed"
        end, name = max(before)
        return f"{at - end} bytes past the end of {name}"


def gen_into_arena(hip_abi, P, num_keys, alphas, root_seeds, beta, beta_mode, fill, offsets=None):
    """dpf_hip_gen_key_batch for the oracle parameters P (of a DPF, or
    oracle.dcf_params for beta_mode 2) into a fresh device arena prefilled with
    `fill`; `alphas`, `root_seeds` and `beta` are device block tensors.  Returns
    the arena after the launch (not synchronised)."""
    H = len(P.log_domain)
    descs = [hip_abi.value_desc(O.leaves(vt), O.is_direct(vt), O.elements_per_block(vt), b)
             for vt, b in zip(P.vtypes, P.blocks_needed)]
    arena = KeygenArena(num_keys, P.tree_levels_needed - 1,
                        [O.elements_per_block(vt) for vt in P.vtypes], fill, offsets=offsets)
    hip_abi.gen_key_batch(num_keys, P.tree_levels_needed - 1, P.hierarchy_to_tree, P.log_domain,
                          P.blocks_needed, descs, alphas, root_seeds, beta, beta_mode,
                          H if beta_mode == 2 else 0,
                          (O.PRG_KEY_LEFT, O.PRG_KEY_RIGHT, O.PRG_KEY_VALUE),
                          arena.tensor("cw_seed"), arena.tensor("cw_left"),
                          arena.tensor("cw_right"), arena.value_corrections())
    return arena


def boundary_key_pairs(num_keys, per_wg, limit=48):
    """The key pairs u // 2 of the lanes u that test_dynamic_chunks_gpu's
    _boundary_items gives for the 2 * num_keys lanes of a key generation launch
    with per_wg chunks per workgroup, thinned to `limit`: the first and the last
    pair, the whole last chunk (cut off where the lane count is no multiple of
    64) and the pair on each side of the two workgroup-range boundaries stay,
    the rest is sampled evenly."""
    from test_dynamic_chunks_gpu import _boundary_items   # imports this module
    n_items = 2 * num_keys
    lanes = _boundary_items(n_items, per_wg)
    pairs = sorted({u // 2 for u in lanes})
    if len(pairs) <= limit:
        return pairs
    span = per_wg * 64
    have = set(lanes)
    keep = {pairs[0], pairs[-1]}
    keep.update(u // 2 for u in range((n_items - 1) // 64 * 64, n_items))
    for u in lanes:
        if u and u % span == 0 and u - 1 in have:
            keep.update(((u - 1) // 2, u // 2))
    assert len(keep) <= limit, (len(keep), limit)
    rest = [k for k in pairs if k not in keep]
    room = limit - len(keep)
    if room >= len(rest):
        keep.update(rest)
    elif room == 1:
        keep.add(rest[len(rest) // 2])
    elif room > 1:
        keep.update(rest[round(j * (len(rest) - 1) / (room - 1))] for j in range(room))
    return sorted(keep)
