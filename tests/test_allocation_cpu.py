"""The allocation probes and the best-split search without a GPU: the four symbols and the ABI version, the layout of
`mcr_allocation_option` as a C compiler sees it, the host-side validation of the three entry points (it runs before a device is
looked for, and leaves every output untouched), `allocation.allocation_records`, and `allocation.search_best_allocation` on
synthetic integer objectives."""

from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.allocation import ALLOCATION_OPTION_FIELDS, DEFAULT_ALLOCATIONS, allocation_records, search_best_allocation

SENTINEL = 0xA5A5A5A5A5A5A5A5
SYMBOLS = ("mcr_probe_allocations_rng", "mcr_probe_allocations_joint_rng", "mcr_probe_allocations_outcomes_rng",
           "mcr_probe_allocations_last_fanout_launches")


@pytest.fixture(scope="module")
def lib():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    return N.load_library()


def _config(**over):
    return Config(**dict(load_config_from_json(os.path.join(REPO, "scenarios", "config.json")), **over))


def test_header_binding_and_library_carry_the_symbols(lib):
    with open(os.path.join(REPO, "include", "mcr.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    declared = set(re.findall(r"\b(mcr_[a-z0-9_]+)\s*\(", hdr))
    for sym in SYMBOLS:
        assert sym in declared and sym in N.ABI_SYMBOLS and hasattr(lib, sym), sym
    exported = subprocess.check_output(["nm", "-D", "--defined-only", N.library_path()], text=True)
    for sym in SYMBOLS:
        assert re.search(rf"\bT {sym}$", exported, re.M), sym
    assert lib.mcr_abi_version() == 8 == N.MCR_ABI_VERSION
    assert lib.mcr_probe_allocations_last_fanout_launches() == 0


def test_the_record_is_four_packed_doubles_as_gcc_sees_it(tmp_path):
    T = N.McrAllocationOption
    assert [f for f, _ in T._fields_] == list(ALLOCATION_OPTION_FIELDS)
    lines = ['printf("size %zu\\n", sizeof(mcr_allocation_option));']
    lines += [f'printf("{f} %zu\\n", offsetof(mcr_allocation_option, {f}));' for f, _ in T._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    seen = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(seen["size"]) == 32 == C.sizeof(T)
    for k, (f, _) in enumerate(T._fields_):
        assert int(seen[f]) == 8 * k == getattr(T, f).offset, f


class _Call:
    """One call of each entry point with HOST sentinel buffers as its outputs: validation comes before the device, so a
    refused call must leave every word of them as it was.  Returns what the three forms answered."""

    WORDS = 64

    def __init__(self, lib, params):
        self.lib, self.params = lib, params

    def __call__(self, options=((1000.0, 10.0, 20.0, 0.5), (2000.0, 0.0, 5.0, 0.25)), n_options=None, null=(), n_paths=64, rng=None):
        n = len(options)
        arr = (N.McrAllocationOption * max(1, n))(*[N.McrAllocationOption(*o) for o in options])
        rng = N.philox_rng(1) if rng is None else rng
        head = lambda: (None if "params" in null else C.byref(self.params), None if "rng" in null else C.byref(rng), 1, 0, n_paths, 120,
                        None if "options" in null else arr, n if n_options is None else n_options)
        answers = []
        for form in ("plain", "joint", "outcomes"):
            bufs = {k: (C.c_uint64 * self.WORDS)(*([SENTINEL] * self.WORDS)) for k in ("counts", "masks", "joint", "extremes", "final", "ruin")}
            counts = None if "counts" in null else C.addressof(bufs["counts"])
            if form == "plain":
                rc = self.lib.mcr_probe_allocations_rng(*head(), counts, 0, None)
            elif form == "joint":
                rc = self.lib.mcr_probe_allocations_joint_rng(*head(), counts, C.addressof(bufs["masks"]), C.addressof(bufs["joint"]),
                                                              C.addressof(bufs["extremes"]), 0, None)
            else:
                rows = N.McrOptionOutcomes(C.addressof(bufs["final"]), C.addressof(bufs["ruin"]), n_paths)
                rc = self.lib.mcr_probe_allocations_outcomes_rng(*head(), counts, C.byref(rows), 0, None)
            msg = N.last_error()
            for k, b in bufs.items():
                assert all(x == SENTINEL for x in b), (form, k, "an output was written")
            assert self.lib.mcr_probe_allocations_last_fanout_launches() == 0
            answers.append((rc, msg))
        return answers


def test_validation_is_host_only_and_leaves_the_outputs_untouched(lib):
    call = _Call(lib, params_from_config(_config()))
    good = (1000.0, 10.0, 20.0, 0.5)
    # each bad field of an option, by name
    cases = [(f, bad) for f in ALLOCATION_OPTION_FIELDS[:3] for bad in (float("nan"), -0.01, float("inf"))]
    cases += [("allocation_inv1_pct", bad) for bad in (-0.1, 1.0000001, float("nan"), float("inf"))]
    for field, bad in cases:
        record = list(good)
        record[ALLOCATION_OPTION_FIELDS.index(field)] = bad
        for rc, msg in call(options=(good, tuple(record), good)):
            assert rc == N.MCR_ERR_INVALID_ARG and msg.startswith(f"options[1].{field} = "), (field, bad, msg)
    # counts and pointers
    for rc, msg in call(n_options=-1):
        assert rc == N.MCR_ERR_INVALID_ARG and "n_options" in msg, msg
    for which in ("options", "counts"):
        for rc, msg in call(null=(which,)):
            assert rc == N.MCR_ERR_INVALID_ARG and "null" in msg, (which, msg)
    for which in ("params", "rng"):
        for rc, msg in call(null=(which,)):
            assert rc == N.MCR_ERR_INVALID_ARG, (which, msg)
    # a bad block: mcr_validate_params' words
    bad_block = params_from_config(_config())
    bad_block.allocation_inv1_pct = 1.5
    assert lib.mcr_validate_params(C.byref(bad_block)) == N.MCR_ERR_INVALID_ARG
    want = N.last_error()
    for rc, msg in _Call(lib, bad_block)():
        assert rc == N.MCR_ERR_INVALID_ARG and msg == want, (msg, want)
    # no options: nothing happens, on any box
    for rc, _ in call(options=()):
        assert rc == 0
    for rc, _ in call(n_options=0):
        assert rc == 0
    # the joint and outcome forms check their own arguments first
    many = tuple(good for _ in range(N.MCR_MAX_JOINT_OPTIONS + 1))
    rc, msg = call(options=many)[1]
    assert rc == N.MCR_ERR_INVALID_ARG and "MCR_MAX_JOINT_OPTIONS" in msg, msg
    arr = (N.McrAllocationOption * 1)(N.McrAllocationOption(*good))
    rng = N.philox_rng(1)
    counts = (C.c_uint64 * 4)(*([SENTINEL] * 4))
    final = (C.c_uint64 * 128)(*([SENTINEL] * 128))
    rc = lib.mcr_probe_allocations_joint_rng(C.byref(call.params), C.byref(rng), 1, 0, 64, 120, arr, 1, C.addressof(counts), None, None, None, 0, None)
    assert rc == N.MCR_ERR_INVALID_ARG and "null joint" in N.last_error()
    rows = N.McrOptionOutcomes(C.addressof(final), None, 63)
    rc = lib.mcr_probe_allocations_outcomes_rng(C.byref(call.params), C.byref(rng), 1, 0, 64, 120, arr, 1, C.addressof(counts), C.byref(rows), 0, None)
    assert rc == N.MCR_ERR_INVALID_ARG and "path_stride" in N.last_error()
    assert all(x == SENTINEL for x in counts) and all(x == SENTINEL for x in final)


def test_allocation_records():
    cfg = _config()
    own = (float(cfg.initial_balance), float(cfg.monthly_contribution), float(cfg.monthly_expenses))
    assert allocation_records(cfg, []) == []
    assert allocation_records(cfg, [0, 0.25, 1]) == [own + (0.0,), own + (0.25,), own + (1.0,)]
    assert allocation_records(cfg, [{"allocation_inv1_pct": 0.4, "monthly_expenses": 1234.5}, {"allocation_inv1_pct": 1.0, "initial_balance": 0}]) == [
        (own[0], own[1], 1234.5, 0.4), (0.0, own[1], own[2], 1.0)]
    assert allocation_records(cfg, DEFAULT_ALLOCATIONS) == [own + (i / 10.0,) for i in range(11)]
    for options, pattern in (
        ([0.5, -0.1], r"allocations\[1\]\.allocation_inv1_pct"),
        ([1.0000001], r"allocations\[0\]\.allocation_inv1_pct"),
        ([0.1, 0.2, float("nan")], r"allocations\[2\]\.allocation_inv1_pct"),
        ([{"monthly_expenses": 5.0}], r"allocations\[0\]\.allocation_inv1_pct is missing"),
        ([{"allocation_inv1_pct": 0.5, "monthly_expenses": -1.0}], r"allocations\[0\]\.monthly_expenses"),
        ([0.5, {"allocation_inv1_pct": 0.5, "initial_balance": float("inf")}], r"allocations\[1\]\.initial_balance"),
        ([{"allocation_inv1_pct": 0.5, "monthly_contribution": float("nan")}], r"allocations\[0\]\.monthly_contribution"),
        ([{"allocation_inv1_pct": 0.5, "inv1_returns_mean": 0.1}], r"allocations\[0\]: unknown key\(s\) \['inv1_returns_mean'\]"),
        (["half"], r"allocations\[0\]\.allocation_inv1_pct = 'half'"),
    ):
        with pytest.raises(ValueError, match=pattern):
            allocation_records(cfg, options)


# ---- the search on synthetic objectives: success COUNTS of 10 000 paths, an integer function of the split ----
N_PATHS = 10_000


def _unit(x):
    return int(round(x * 100))


OBJECTIVES = {
    # name: (count as a function of the split in hundredths, the config's own split, the answer)
    "single_peak_at_0.37": (lambda u: 9000 - 3 * (u - 37) ** 2, 0.6, 0.37),
    "maximum_at_0": (lambda u: 9000 - 40 * u, 0.6, 0.0),
    "maximum_at_1": (lambda u: 5000 + 40 * u, 0.6, 1.0),
    "flat_plateau": (lambda u: 7777, 0.6, 0.6),                                     # every point ties: the config's own split
    "flat_plateau_own_off_grid": (lambda u: 7777, 0.33, 0.33),                      # ... which round 2 and 3 reach (0.3 -> 0.32, 0.34 -> 0.33)
    "two_equal_peaks": (lambda u: 9000 - 5 * min(abs(u - 20), abs(u - 80)) ** 2, 0.6, 0.8),    # the peak nearer 0.6
    "two_equal_peaks_equidistant": (lambda u: 9000 - 5 * min(abs(u - 20), abs(u - 80)) ** 2, 0.5, 0.2),   # then the lower
    # 0.2 and 0.4 are equally far from 0.3, although |0.2 - 0.3| and |0.4 - 0.3| differ in their last bits as doubles: the lower
    "two_equal_peaks_around_own_0.3": (lambda u: 9000 - 5 * min(abs(u - 20), abs(u - 40)) ** 2, 0.3, 0.2),
    "peak_between_grid_points": (lambda u: 9000 - 7 * abs(u - 45), 0.6, 0.45),
}


def _first(seen, own):
    """The tie rule on `seen` = {split: probability}: the highest probability, then the split nearest `own` (distances in
    hundredths, as integers where `own` is one), then the lower."""
    return min(seen, key=lambda s: (-seen[s], abs(_unit(s) - _unit(own)) if own == _unit(own) / 100.0 else abs(s - own), s))


class _Joint:
    def __init__(self, splits, count):
        self.splits, self.count = list(splits), count

    def indistinguishable_from(self, a):
        top = self.count(_unit(self.splits[a]))
        return [b for b, s in enumerate(self.splits) if b == a or top - self.count(_unit(s)) < 25]


@pytest.mark.parametrize("name", list(OBJECTIVES))
def test_search_on_a_synthetic_objective(name):
    count, own, answer = OBJECTIVES[name]
    calls, joint_calls, events = [], [], []

    def probe(splits):
        calls.append(list(splits))
        return [100.0 * count(_unit(s)) / N_PATHS for s in splits]

    def probe_joint(splits):
        joint_calls.append(list(splits))
        return _Joint(splits, count)

    best, prob, curve, tied = search_best_allocation(probe, own, on_level=events.append, probe_joint=probe_joint)
    assert best == answer and prob == 100.0 * count(_unit(answer)) / N_PATHS, (best, prob)
    # three probes at the default resolution, at most 15 points each, none twice, each a multiple of the resolution
    assert len(calls) == 3 and all(1 <= len(c) <= 15 for c in calls), [len(c) for c in calls]
    flat = [s for c in calls for s in c]
    assert len(set(flat)) == len(flat)
    assert all(0.0 <= s <= 1.0 and s == _unit(s) / 100.0 for s in flat)
    assert calls[0] == [i / 10.0 for i in range(11)]
    # rounds 2 and 3: steps 0.02 and 0.01, strictly inside (best - step, best + step) of the best point before them
    seen = {}
    for r, c in enumerate(calls):
        if r:
            top = _first(seen, own)
            before, step = (0.1, 0.02) if r == 1 else (0.02, 0.01)
            for s in c:
                assert abs(s - top) < before - 1e-9 and abs(round((s - top) / step) - (s - top) / step) < 1e-9, (r, s, top)
        seen.update({s: 100.0 * count(_unit(s)) / N_PATHS for s in c})
    # the answer is the best of ALL evaluated points under the tie rule
    assert best == _first(seen, own)
    assert curve == [{"allocation_inv1_pct": s, "probability": seen[s]} for s in flat]
    # the events: one per point, in order, with the round and the bracket being refined
    assert [e["allocation_inv1_pct"] for e in events] == flat
    assert all(list(e) == ["type", "iteration", "allocation_inv1_pct", "probability", "lo", "hi"] for e in events)
    assert {e["type"] for e in events} == {"allocation_search_iter"}
    assert [e["iteration"] for e in events] == [r + 1 for r, c in enumerate(calls) for _ in c]
    assert all(e["probability"] == round(seen[e["allocation_inv1_pct"]], 2) for e in events)
    assert all(e["lo"] is None and e["hi"] is None for e in events if e["iteration"] == 1)
    assert all(e["lo"] <= e["allocation_inv1_pct"] <= e["hi"] and 0.0 <= e["lo"] < e["hi"] <= 1.0 for e in events if e["iteration"] > 1)
    # one joint probe over the first grid and the answer; tied holds the answer
    assert joint_calls == [sorted(set(calls[0]) | {best})]
    assert best in tied and set(tied) <= set(joint_calls[0])
    if name.startswith("flat_plateau"):
        assert tied == joint_calls[0]
    # deterministic; and without the joint probe the answer stands alone
    assert search_best_allocation(probe, own)[:3] == (best, prob, curve)
    assert search_best_allocation(probe, own)[3] == [best]


def test_search_arguments():
    probe = lambda splits: [50.0 for _ in splits]
    with pytest.raises(ValueError, match="resolution"):
        search_best_allocation(probe, 0.5, resolution=0.0)
    with pytest.raises(ValueError, match="resolution"):
        search_best_allocation(probe, 0.5, resolution=0.03)
    with pytest.raises(ValueError, match="own_allocation"):
        search_best_allocation(probe, 1.5)
    with pytest.raises(ValueError, match="levels_per_call"):
        search_best_allocation(probe, 0.5, levels_per_call=0)
    # a coarse resolution ends with the first grid; a fine one takes one more round; a small probe splits a round
    calls = []
    counted = lambda splits: calls.append(list(splits)) or [100.0 - abs(s - 0.3333) for s in splits]
    assert search_best_allocation(counted, 0.5, resolution=0.1)[0] == 0.3 and len(calls) == 1
    del calls[:]
    best = search_best_allocation(counted, 0.5, resolution=0.001)[0]
    assert best == 0.333 and len(calls) == 4 and all(len(c) <= 15 for c in calls)
    assert len({s for c in calls for s in c}) == sum(len(c) for c in calls)
    del calls[:]
    assert search_best_allocation(counted, 0.5, levels_per_call=4)[0] == 0.33 and all(len(c) <= 4 for c in calls)
    # one or two levels a call: less than one point a side of the best, so the step halves (0.1 -> 0.05 -> 0.03 -> 0.02 -> 0.01)
    for L in (1, 2, 3):
        del calls[:]
        best, prob, curve, tied = search_best_allocation(counted, 0.5, levels_per_call=L)
        assert best == 0.33 and prob == 100.0 - abs(0.33 - 0.3333) and tied == [0.33], (L, best)
        assert calls and all(1 <= len(c) <= L for c in calls), (L, [len(c) for c in calls])
        flat = [s for c in calls for s in c]
        assert len(set(flat)) == len(flat) and flat[:11] == [i / 10.0 for i in range(11)] and len(flat) <= 11 + 2 * 7
        assert [c["allocation_inv1_pct"] for c in curve] == flat
    # a maximum at either end and a flat curve end too
    for L in (1, 2):
        assert search_best_allocation(lambda splits: [100.0 * s for s in splits], 0.5, levels_per_call=L)[0] == 1.0
        assert search_best_allocation(lambda splits: [100.0 - 100.0 * s for s in splits], 0.5, levels_per_call=L)[0] == 0.0
        assert search_best_allocation(probe, 0.47, levels_per_call=L)[0] == 0.47


def test_cli_refuses_conflicting_and_malformed_allocation_flags():
    """examples/run_scenario.py: every refusal comes from the argument parser, before a simulator exists (exit status 2)."""
    import sys

    base = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
            os.path.join(REPO, "scenarios", "config.json")]
    for extra, words in (
        (["--allocations", "0.2,0.8"], "need --working-months"),
        (["--best-allocation"], "need --working-months"),
        (["--working-months", "240", "--allocations", "0.2", "--best-allocation"], "separate questions"),
        (["--working-months", "240", "--best-allocation", "--cohorts"], "the other questions are separate"),
        (["--working-months", "240", "--best-allocation", "--frontier", "180,240"], "the other questions are separate"),
        (["--working-months", "240", "--allocations", "0.5", "--earliest-retirement"], "the other questions are separate"),
        (["--working-months", "240", "--allocations", "0.5", "--max-expenses"], "the other questions are separate"),
        (["--working-months", "240", "--allocations", "0.5", "--stress"], "the other questions are separate"),
        (["--working-months", "240", "--allocations", ","], "at least one value"),
        (["--working-months", "240", "--allocations", "0.2,x"], "comma-separated numbers"),
        (["--working-months", "240", "--best-allocation", "--allocation-resolution", "0.03"], "must be a whole number"),
        (["--working-months", "240", "--best-allocation", "--allocation-resolution", "0"], "must be a whole number"),
        (["--working-months", "240", "--best-allocation", "--paired"], "--paired goes with"),
        (["--working-months", "240", "--allocation-resolution", "0.05"], "goes with --best-allocation"),
    ):
        r = subprocess.run(base + extra, cwd=REPO, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and words in r.stderr, (extra, r.returncode, r.stderr[-400:])
