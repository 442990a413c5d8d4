"""The chunk schedule of the full-domain expand launches (dpf_hip_octet_schedule,
plan_chunks in dpf_expand_plan.hip): a pure function of the launch's shape, the CU
count and the DPF_OCTET_* hooks, so it is checked here without a GPU.
"""
import itertools
import json
import os
import subprocess
import sys

import pytest

from distributed_point_functions_amd import hip_abi as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("DPF_OCTET_DYNAMIC", "DPF_OCTET_TAPER", "DPF_OCTET_GLOBAL", "DPF_OCTET_TAPER_AT",
         "DPF_OCTET_WALK")
WAVES_PER_WG = 16
# items 2^16 .. 2^24, with odd numbers of start seeds (3, 5 and 7 x 2^k) among them.
ITEMS = [1 << 16, 1 << 17, 3 << 16, 5 << 17, 1 << 20, 7 << 18, 1 << 22, 3 << 22, 1 << 24]
CUS = [1, 4, 16, 64, 256]          # waves 16 .. 4096
DEPTHS = range(1, 14)


@pytest.fixture(autouse=True)
def _hooks(monkeypatch):
    """No hook set, but the chip-wide counter and both finer phases on at every
    size (unset, they are on only for large launches: test_defaults_by_size)."""
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    monkeypatch.setenv("DPF_OCTET_TAPER", "2")
    monkeypatch.setenv("DPF_OCTET_GLOBAL", "1")


def _grid():
    return itertools.product(ITEMS, DEPTHS, (1, 3), CUS)


def _shift_today(S):
    """DPF_OCTET_DYNAMIC unset: 4 levels off subtrees of >= 11, else 2."""
    return 4 if S >= 11 else 2


def _dynamic_today(items, S, min_s, cus, sh):
    """The condition under which a launch gets dynamic 64-item chunks."""
    return (S - sh >= min_s and (items << sh) % (cus * 64) == 0
            and (items << sh) >= 4 * cus * 1024)


def _check_tiling(plan, items, S, min_s):
    """Phases tile the leaf-block range [0, items << S) once, in order."""
    pos = 0
    for j, ph in enumerate(plan["phases"]):
        assert ph["depth"] >= min_s
        assert ph["chunks"] > 0
        assert (ph["first_item"] << ph["depth"]) == pos, (j, plan)
        pos += (ph["chunks"] * 64) << ph["depth"]
    assert pos == items << S, plan


def test_phases_tile_the_domain_once():
    k0 = 9
    seen_phases = set()
    for items, S, min_s, cus in _grid():
        plan = H.octet_schedule(items, k0, S, min_s, cus)
        sh = _shift_today(S)
        if not _dynamic_today(items, S, min_s, cus, sh):
            # too small for dynamic chunks (or not divisible): static, no taper
            assert plan["shift"] == 0 and plan["phases"] == [], (items, S, min_s, cus)
            continue
        assert plan["shift"] == sh
        assert plan["global"] and plan["counters"] == 1
        _check_tiling(plan, items, S, min_s)
        depths = [ph["depth"] for ph in plan["phases"]]
        assert depths == sorted(depths, reverse=True)            # coarse first
        for ph in plan["phases"]:
            j = (S - sh - ph["depth"]) // 2
            assert ph["depth"] == S - sh - 2 * j and ph["k0"] == k0 + sh + 2 * j
            assert ph["k0"] + ph["depth"] == k0 + S
        seen_phases.add(len(plan["phases"]))
    assert seen_phases == {1, 2, 3}


def test_boundaries_follow_the_rule():
    """A phase hands over when <= 2 of its chunks per resident wave are left."""
    for items, S, min_s, cus in _grid():
        plan = H.octet_schedule(items, 0, S, min_s, cus)
        if not plan["shift"]:
            continue
        waves = cus * WAVES_PER_WG
        s0 = S - plan["shift"]
        by_depth = {ph["depth"]: ph for ph in plan["phases"]}
        coarse = (items << plan["shift"]) // 64
        if s0 - 2 >= min_s:
            tail0 = min(coarse, 2 * waves)                   # phase-0 chunks left to finer phases
            assert by_depth.get(s0, {"chunks": 0})["chunks"] == coarse - tail0
            if s0 - 4 >= min_s:
                tail1 = min(tail0 * 4, 2 * waves)            # phase-1 chunks left to phase 2
                assert by_depth[s0 - 2]["chunks"] == tail0 * 4 - tail1
                assert by_depth[s0 - 4]["chunks"] == tail1 * 4
            else:
                assert by_depth[s0 - 2]["chunks"] == tail0 * 4
                assert s0 - 4 not in by_depth
        else:
            assert list(by_depth) == [s0]


def test_config_shapes():
    """The two sizes the schedule was derived for (256 CUs)."""
    # 2^30 uint64 outputs: 2^29 leaf blocks, S = 11 -> 7 for the bulk, the
    # last 1/8 at 5 (2 of 16 chunks per wave), the last 1/32 at 3 (2 of the 8
    # depth-5 chunks per wave that the 1/8 makes).
    plan = H.octet_schedule(1 << 18, 18, 11, 3, 256)
    assert [ph["depth"] for ph in plan["phases"]] == [7, 5, 3]
    total = 1 << 29
    assert [(ph["chunks"] * 64) << ph["depth"] for ph in plan["phases"]] == [
        total - total // 8, total // 8 - total // 32, total // 32]
    # the 2^27-output shard: S = 8 -> 6, the last half at 4, no phase at 2.
    plan = H.octet_schedule(1 << 18, 15, 8, 3, 256)
    assert [ph["depth"] for ph in plan["phases"]] == [6, 4]
    assert [(ph["chunks"] * 64) << ph["depth"] for ph in plan["phases"]] == [1 << 25, 1 << 25]


def test_taper_hook_caps_the_finer_phases(monkeypatch):
    for taper in (0, 1, 2):
        monkeypatch.setenv("DPF_OCTET_TAPER", str(taper))
        for items, S, min_s, cus in _grid():
            plan = H.octet_schedule(items, 3, S, min_s, cus)
            if not plan["shift"]:
                continue
            assert 1 <= len(plan["phases"]) <= taper + 1
            _check_tiling(plan, items, S, min_s)
            assert min(ph["depth"] for ph in plan["phases"]) >= S - plan["shift"] - 2 * taper


def test_taper_at_hook_moves_the_boundary(monkeypatch):
    monkeypatch.setenv("DPF_OCTET_TAPER_AT", "1")
    plan = H.octet_schedule(1 << 18, 15, 8, 3, 256)
    assert [(ph["chunks"] * 64) << ph["depth"] for ph in plan["phases"]] == [3 << 24, 1 << 24]


@pytest.mark.parametrize("dynamic", ["", "2", "4"])
def test_hooks_off_reproduce_the_uniform_shape(monkeypatch, dynamic):
    """DPF_OCTET_TAPER=0 with DPF_OCTET_GLOBAL=0: one phase of the shape the
    launch had before the schedule existed -- (items << shift) / (cus * 64)
    chunks per workgroup of subtrees `shift` levels shallower."""
    monkeypatch.setenv("DPF_OCTET_TAPER", "0")
    monkeypatch.setenv("DPF_OCTET_GLOBAL", "0")
    if dynamic:
        monkeypatch.setenv("DPF_OCTET_DYNAMIC", dynamic)
    for items, S, min_s, cus in _grid():
        plan = H.octet_schedule(items, 5, S, min_s, cus)
        sh = int(dynamic) if dynamic else _shift_today(S)
        if not _dynamic_today(items, S, min_s, cus, sh):
            assert plan["shift"] == 0
            continue
        assert plan["shift"] == sh and not plan["global"] and plan["counters"] == cus
        (ph,) = plan["phases"]
        assert ph == {"chunks": (items << sh) // 64, "first_item": 0, "k0": 5 + sh,
                      "depth": S - sh}
        assert ph["chunks"] % cus == 0


def test_per_workgroup_counters_share_every_phase(monkeypatch):
    """DPF_OCTET_GLOBAL=0 keeps the phase boundaries; every workgroup takes an
    equal share of each phase."""
    for items, S, min_s, cus in _grid():
        monkeypatch.setenv("DPF_OCTET_GLOBAL", "1")
        a = H.octet_schedule(items, 0, S, min_s, cus)
        monkeypatch.setenv("DPF_OCTET_GLOBAL", "0")
        b = H.octet_schedule(items, 0, S, min_s, cus)
        assert a["phases"] == b["phases"] and a["shift"] == b["shift"]
        if b["shift"]:
            assert b["counters"] == cus and all(ph["chunks"] % cus == 0 for ph in b["phases"])


def test_defaults_by_size(monkeypatch):
    """Unset, the chip-wide counter and the taper apply from 2^20 leaf blocks
    per CU (where they measured faster than the uniform per-workgroup shape)."""
    monkeypatch.delenv("DPF_OCTET_TAPER")
    monkeypatch.delenv("DPF_OCTET_GLOBAL")
    for levels, S, phases in ((29, 11, 3), (28, 10, 3), (27, 9, 1), (26, 8, 1)):
        plan = H.octet_schedule(1 << (levels - S), levels - S, S, 3, 256)
        assert plan["shift"] and len(plan["phases"]) == phases, (levels, plan)
        assert plan["global"] == (levels >= 28) and plan["counters"] == (1 if levels >= 28 else 256)


def test_dynamic_off_is_static(monkeypatch):
    monkeypatch.setenv("DPF_OCTET_DYNAMIC", "0")
    for items, S, min_s, cus in _grid():
        assert H.octet_schedule(items, 0, S, min_s, cus) == {
            "shift": 0, "global": False, "counters": 0, "phases": []}


def test_last_expand_schedule_before_any_launch():
    """Process-wide state, so a fresh process is asked: it loads the library,
    launches nothing and prints last_expand_schedule()."""
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); "
            "from distributed_point_functions_amd import hip_abi as H; "
            "print(json.dumps(H.last_expand_schedule()))")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {
        "shift": 0, "global": False, "counters": 0, "phases": []}


def test_rejects_bad_shapes():
    for bad in ((0, 0, 5, 3, 256), (1 << 20, -1, 5, 3, 256), (1 << 20, 60, 5, 3, 256),
                (1 << 20, 0, 5, 3, 0)):
        with pytest.raises(H.DpfHipError):
            H.octet_schedule(*bad)
