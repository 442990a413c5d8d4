"""The chip-wide chunk counter and the tapered chunks of the full-domain expand
kernels (dpf_expand_plan.hip, "Who takes which chunk") give the static launch's
bytes.

Every schedule is compared byte for byte with the static one-item-per-thread
launch (DPF_OCTET_DYNAMIC=0), which tests/test_kernels_gpu.py and the full-size
tests tie to the oracle.  Every launch writes into the caller's buffer, filled
with a nonzero pattern first, so a chunk that no wave took shows up as a
difference instead of as the previous launch's correct bytes.
"""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

M32 = 4294967291
M64 = 18446744073709551557
HOOKS = ("DPF_OCTET_DYNAMIC", "DPF_OCTET_TAPER", "DPF_OCTET_GLOBAL", "DPF_OCTET_TAPER_AT",
         "DPF_OCTET_WALK", "DPF_EXPAND_TOP", "DPF_EXPAND_NO_OCTET")


@pytest.fixture(scope="module")
def hip():
    import torch
    from distributed_point_functions_amd import hip_abi
    hip_abi.load(require_gpu=True)
    assert torch.cuda.is_available()
    return hip_abi


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)


def _rand_value(rng, vt):
    out = []
    for kind, bits, mod in O.leaves(vt):
        if kind == O.LEAF_INTMODN:
            out.append(int(rng.integers(0, 2**62)) % mod)
        else:
            out.append(int.from_bytes(rng.bytes(bits // 8), "little"))
    return out


def _args(hip, rng, vt, levels, starts, party):
    b = (O.bits_needed(vt, 40.0) + 127) // 128
    E = O.elements_per_block(vt)
    blocks = lambda n: rng.integers(0, 2**64, size=(n, 2), dtype=np.uint64)
    desc = hip.value_desc(O.leaves(vt), O.is_direct(vt), E, b)
    return (hip.to_device_blocks(blocks(starts)),
            hip.to_device_u8(rng.integers(0, 2, size=starts, dtype=np.uint8)),
            hip.to_device_blocks(blocks(levels)),
            hip.to_device_u8(rng.integers(0, 2, size=levels, dtype=np.uint8)),
            hip.to_device_u8(rng.integers(0, 2, size=levels, dtype=np.uint8)),
            (O.PRG_KEY_LEFT, O.PRG_KEY_RIGHT, O.PRG_KEY_VALUE), desc, E,
            hip.to_device_blocks(O._leaf_array([_rand_value(rng, vt) for _ in range(E)])), party)


def _expand_into(hip, args, buf, stream=None):
    """One expansion into `buf`, which holds a nonzero pattern until it is written."""
    buf.fill_(0xA5)
    out = hip.expand(*args, out=buf, stream=stream)
    assert out.data_ptr() == buf.data_ptr()
    return out


def _static(hip, monkeypatch, args, kernel):
    """The static launch's output: the reference of every mode of one shape."""
    import torch
    monkeypatch.setenv("DPF_OCTET_DYNAMIC", "0")
    want = hip.expand(*args)
    torch.cuda.synchronize()
    assert hip.last_expand_kernel()[0].startswith(kernel)
    assert hip.last_expand_schedule()["shift"] == 0
    monkeypatch.delenv("DPF_OCTET_DYNAMIC")
    return want


def _check_modes(hip, monkeypatch, args, want, modes, finer, depth):
    """`finer`: the finer phases the shape allows; `depth`: phase 0's subtree
    depth.  Every mode must have run, on this device, the schedule it names
    (dpf_hip_last_expand_schedule): a launch that fell back to the static
    shape would compare static with static."""
    import torch
    buf = torch.empty_like(want)
    for mode in modes:
        for k, v in mode.items():
            monkeypatch.setenv(k, v)
        got = _expand_into(hip, args, buf)
        torch.cuda.synchronize()
        ran = hip.last_expand_schedule()
        assert ran["shift"] > 0, (mode, ran)
        assert ran["phases"][0]["depth"] == depth, (mode, ran)
        if "DPF_OCTET_GLOBAL" in mode:
            want_global = mode["DPF_OCTET_GLOBAL"] == "1"
            assert ran["global"] == want_global and (ran["counters"] == 1) == want_global, (mode, ran)
        if "DPF_OCTET_TAPER" in mode:
            assert len(ran["phases"]) == 1 + min(int(mode["DPF_OCTET_TAPER"]), finer), (mode, ran)
            assert [ph["depth"] for ph in ran["phases"]] == [
                depth - 2 * j for j in range(len(ran["phases"]))], (mode, ran)
        assert torch.equal(got, want), mode
        for k in mode:
            monkeypatch.delenv(k)


def _grid(dynamic=None, extra=None):
    """Every DPF_OCTET_TAPER x DPF_OCTET_GLOBAL mode, then the defaults."""
    modes = []
    for taper in ("0", "1", "2"):
        for glob in ("0", "1"):
            m = {"DPF_OCTET_TAPER": taper, "DPF_OCTET_GLOBAL": glob}
            if dynamic:
                m["DPF_OCTET_DYNAMIC"] = dynamic
            modes.append(m)
    # hooks unset: on from 2^20 leaf blocks per CU, else the uniform shape
    modes.append({"DPF_OCTET_DYNAMIC": dynamic} if dynamic else {})
    return modes + (extra or [])


def test_uint64_26_levels_one_finer_phase(hip, monkeypatch):
    # 2^26 leaf blocks (1 GiB): dynamic with shift 2, S 8 -> 6, then 4.
    vt = ("int", 64)
    args = _args(hip, np.random.default_rng(2601), vt, 26, 1, 1)
    want = _static(hip, monkeypatch, args, "octet/")
    _check_modes(hip, monkeypatch, args, want,
                 _grid(extra=[{"DPF_OCTET_TAPER_AT": "1"}, {"DPF_OCTET_WALK": "0"}]),
                 finer=1, depth=6)


def test_uint64_27_levels_both_finer_phases(hip, monkeypatch):
    # 2^27 leaf blocks (2 GiB), DPF_OCTET_DYNAMIC=2: S 9 -> 7 -> 5 -> 3.
    vt = ("int", 64)
    args = _args(hip, np.random.default_rng(2702), vt, 27, 1, 0)
    want = _static(hip, monkeypatch, args, "octet/")
    _check_modes(hip, monkeypatch, args, want, _grid(dynamic="2"), finer=2, depth=7)


@pytest.mark.parametrize("party", [0, 1])
def test_24_levels_four_starts(hip, monkeypatch, party):
    # The finer phases cover whole start seeds (the last half of the domain)
    # or end inside one (DPF_OCTET_TAPER_AT=1: the last quarter).
    vt = ("int", 64)
    args = _args(hip, np.random.default_rng(2400 + party), vt, 24, 4, party)
    want = _static(hip, monkeypatch, args, "octet/")
    _check_modes(hip, monkeypatch, args, want,
                 _grid(extra=[{"DPF_OCTET_TAPER_AT": "1", "DPF_OCTET_TAPER": "2"},
                              {"DPF_OCTET_TAPER_AT": "1", "DPF_OCTET_TAPER": "2",
                               "DPF_OCTET_GLOBAL": "0"}]),
                 finer=1, depth=6)


@pytest.mark.parametrize("vt", [("tuple", [("intmodn", 32, M32)] * 2),
                                ("tuple", [("int", 32), ("int", 64)])], ids=str)
def test_tuples_26_levels(hip, monkeypatch, vt):
    # Mod32Leaf's parked pair and SwarLeaf under a subtree depth that varies
    # from chunk to chunk.
    args = _args(hip, np.random.default_rng(len(str(vt))), vt, 26, 1, 1)
    want = _static(hip, monkeypatch, args, "octet/")
    _check_modes(hip, monkeypatch, args, want, _grid(), finer=1, depth=6)


@pytest.mark.parametrize("vt,levels", [(("int", 64), 24), (("tuple", [("intmodn", 64, M64)] * 2), 24),
                                       (("int", 64), 25)], ids=str)
def test_pair_kernel(hip, monkeypatch, vt, levels):
    # expand_kernel's minimum subtree depth is 1: 24 levels give S 6 -> 4 -> 2,
    # 25 levels S 7 -> 5 -> 3 -> 1 (both finer phases).
    monkeypatch.setenv("DPF_EXPAND_NO_OCTET", "1")
    args = _args(hip, np.random.default_rng(levels), vt, levels, 1, 0)
    want = _static(hip, monkeypatch, args, "pair/")
    _check_modes(hip, monkeypatch, args, want, _grid(), finer=levels - 23, depth=levels - 20)


def test_two_streams_have_their_own_counters(hip, monkeypatch):
    import torch
    vt = ("int", 64)
    # 26 levels: S 8 -> 6, then 4, so both launches also taper at once.
    a = _args(hip, np.random.default_rng(11), vt, 26, 1, 0)
    b = _args(hip, np.random.default_rng(12), vt, 26, 1, 1)
    want_a = _static(hip, monkeypatch, a, "octet/")
    want_b = _static(hip, monkeypatch, b, "octet/")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    buf_a, buf_b = torch.empty_like(want_a), torch.empty_like(want_b)
    buf_a.fill_(0xA5)
    buf_b.fill_(0xA5)
    torch.cuda.synchronize()
    monkeypatch.setenv("DPF_OCTET_GLOBAL", "1")     # one counter per launch
    monkeypatch.setenv("DPF_OCTET_TAPER", "2")
    for _ in range(3):
        hip.expand(*a, out=buf_a, stream=s1)
        hip.expand(*b, out=buf_b, stream=s2)
    torch.cuda.synchronize()
    ran = hip.last_expand_schedule()
    assert ran["global"] and [ph["depth"] for ph in ran["phases"]] == [6, 4], ran
    assert torch.equal(buf_a, want_a)
    assert torch.equal(buf_b, want_b)
