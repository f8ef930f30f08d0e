"""The required-starting-balance search (monte_carlo_retirement_amd/nestegg.py) against stub probes, its lock-step form, the
scenario-key check of `success_probability_by_scenarios`, and the new C entry point's declaration and binding."""

from __future__ import annotations

import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.nestegg import (INITIAL_BALANCE_CAP, SCENARIO_FIELDS, scenario_records,
                                                search_minimum_initial_balance, search_minimum_initial_balance_many)


class Stub:
    """probe_levels(levels) -> [%] from a function of the level; records the calls."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, levels):
        self.calls.append(list(levels))
        return [self.fn(x) for x in levels]


def step(threshold):
    return lambda x: 90.0 if x >= threshold else 10.0


@pytest.mark.parametrize("threshold,start", [(345678.9, 100000.0), (1.0, 1.0), (0.37, 5.0), (98765432.1, 0.0), (250000.0, 250000.0)])
@pytest.mark.parametrize("L", [1, 2, 8, 15])
def test_monotone_step_is_found_to_the_resolution(threshold, start, L):
    probe = Stub(step(threshold))
    x, p, curve = search_minimum_initial_balance(probe, 85.0, start, levels_per_call=L, resolution=1.0)
    assert x - 1.0 - 1e-9 < threshold <= x
    assert p == 90.0
    assert all(len(c) <= L for c in probe.calls)
    below = max(c["initial_balance"] for c in curve if c["initial_balance"] < x)
    assert x - below <= 1.0 + 1e-9 and probe.fn(below) < 85.0


@pytest.mark.parametrize("threshold", [0.01, 12.34, 123456.78, 9876543.21])
def test_step_gives_the_exact_cent(threshold):
    x, p, _ = search_minimum_initial_balance(Stub(step(threshold)), 85.0, 1000.0, levels_per_call=15, resolution=0.01)
    assert x == threshold and p == 90.0


def test_probe_count_bound():
    """bracket + ceil(log_{L+1}(range / resolution)) calls"""
    for L in (1, 2, 4, 8, 15):
        for threshold in (0.5, 77.7, 500000.0, 12345678.9):
            probe = Stub(step(threshold))
            search_minimum_initial_balance(probe, 85.0, 1000.0, levels_per_call=L, resolution=1.0)
            rungs = [0.0] + [1000.0 * 2 ** k for k in range(40)]
            first_hit = next(i for i, r in enumerate(rungs) if r >= threshold)
            bracket = math.ceil((first_hit + 1) / L)
            lo, hi = rungs[first_hit - 1], rungs[first_hit]
            refine = math.ceil(math.log(max(hi - lo, 1.0) / 1.0) / math.log(L + 1) - 1e-12)
            assert len(probe.calls) <= bracket + refine, (L, threshold, probe.calls)


def _noisy(seed):
    rng = np.random.default_rng(seed)
    noise = {}

    def fn(x):   # rising curve with large, deterministic per-level noise: many local reversals
        if x not in noise:
            noise[x] = rng.normal(0.0, 4.0)
        return float(np.clip(20.0 + x / 5000.0 + noise[x], 0.0, 100.0))

    return fn


@pytest.mark.parametrize("seed", range(6))
def test_noisy_non_monotone_keeps_the_invariant(seed):
    probe = Stub(_noisy(seed))
    target = 80.0
    x, p, curve = search_minimum_initial_balance(probe, target, 10000.0, levels_per_call=8, resolution=0.5)
    seen = {c["initial_balance"]: c["probability"] for c in curve}
    assert seen[x] == p >= target
    lo = max(v for v in seen if v < x)
    assert seen[lo] < target and x - lo <= 0.5 + 1e-9
    assert len(seen) == len(curve)   # every level evaluated once


def test_target_met_at_zero_returns_zero():
    probe = Stub(lambda x: 95.0)
    x, p, curve = search_minimum_initial_balance(probe, 85.0, 200000.0, levels_per_call=15)
    assert (x, p) == (0.0, 95.0)
    assert len(probe.calls) == 1 and probe.calls[0][0] == 0.0 and curve[0] == {"initial_balance": 0.0, "probability": 95.0}


def test_never_reaching_returns_minus_one_and_warns():
    probe = Stub(lambda x: 10.0 + x * 1e-10)
    with pytest.warns(RuntimeWarning, match="cap"):
        x, p, curve = search_minimum_initial_balance(probe, 85.0, 3000.0, levels_per_call=15)
    assert INITIAL_BALANCE_CAP == 1e11
    assert x == -1.0 and p == probe.fn(INITIAL_BALANCE_CAP)
    assert max(c["initial_balance"] for c in curve) == INITIAL_BALANCE_CAP


def test_levels_are_whole_cents_and_curve_and_events_have_their_shape():
    events = []
    probe = Stub(step(1234.567))
    x, p, curve = search_minimum_initial_balance(probe, 85.0, 333.333, levels_per_call=4, resolution=0.01, on_level=events.append)
    assert all(v == round(v, 2) for call in probe.calls for v in call)
    assert x == 1234.57
    assert [c["initial_balance"] for c in curve] == [v for call in probe.calls for v in call]
    assert all(set(c) == {"initial_balance", "probability"} for c in curve)
    assert len(events) == len(curve)
    assert {e["type"] for e in events} == {"initial_balance_search_iter"}
    assert all(set(e) == {"type", "iteration", "initial_balance", "probability", "target", "lo", "hi"} for e in events)
    assert [e["iteration"] for e in events] == [i + 1 for i, call in enumerate(probe.calls) for _ in call]
    assert curve[0]["initial_balance"] == 0.0 and curve[1]["initial_balance"] == 333.33


def test_argument_checks():
    for kw in ({"levels_per_call": 0}, {"resolution": 0.0}, {"resolution": -1.0}):
        with pytest.raises(ValueError):
            search_minimum_initial_balance(Stub(step(1.0)), 85.0, 1.0, **kw)
        with pytest.raises(ValueError):
            search_minimum_initial_balance_many(lambda rows, levels: [], 85.0, [1.0], **kw)
    with pytest.raises(ValueError):
        search_minimum_initial_balance_many(lambda rows, levels: [], 85.0, [1.0, 2.0], monthly_expenses=[1.0])


def test_many_equals_the_single_searches_with_one_probe_call_a_round():
    # searches of different lengths: a step met at 0, steps far apart, a noisy curve, one that never reaches the cap
    fns = [lambda x: 95.0, step(345.67), step(8_765_432.1), _noisy(3), step(0.02), lambda x: 10.0]
    starts = [5000.0, 1.0, 100000.0, 10000.0, 250.0, 1e9]
    target = 80.0
    singles, single_events, single_calls = [], [], []
    for fn, s in zip(fns, starts):
        ev, probe = [], Stub(fn)
        with pytest.warns(RuntimeWarning) if fn is fns[-1] else _no_warning():
            singles.append(search_minimum_initial_balance(probe, target, s, levels_per_call=7, resolution=1.0, on_level=ev.append))
        single_events.append(ev)
        single_calls.append(probe.calls)
    rounds = []

    def probe_rows(rows, levels_2d):
        rounds.append((list(rows), [list(r) for r in levels_2d]))
        return [[fns[i](x) for x in levels] for i, levels in zip(rows, levels_2d)]

    events = []
    expenses = [1000.0 * (i + 1) for i in range(len(fns))]
    with pytest.warns(RuntimeWarning, match="cap"):
        many = search_minimum_initial_balance_many(probe_rows, target, starts, levels_per_call=7, resolution=1.0,
                                                   on_level=events.append, monthly_expenses=expenses)
    assert many == singles
    assert many[0][0] == 0.0 and many[-1][0] == -1.0
    # one probe call per round: as many rounds as the longest single search made calls, and each search saw exactly its own calls
    assert len(rounds) == max(len(c) for c in single_calls)
    for i, calls in enumerate(single_calls):
        mine = [levels[rows.index(i)] for rows, levels in rounds if i in rows]
        assert mine == calls
    assert all(rows == sorted(rows) for rows, _ in rounds)
    for i, ev in enumerate(single_events):   # the events of search i, tagged with its spending level
        assert [e for e in events if e["monthly_expenses"] == expenses[i]] == [dict(e, monthly_expenses=expenses[i]) for e in ev]
    # untagged without the spending levels
    ev2 = []
    search_minimum_initial_balance_many(probe_rows, target, starts[:2], levels_per_call=7, on_level=ev2.append)
    assert ev2 and all("monthly_expenses" not in e for e in ev2)
    assert search_minimum_initial_balance_many(probe_rows, target, []) == []


class _no_warning:
    def __enter__(self):
        import warnings

        self._c = warnings.catch_warnings()
        self._c.__enter__()
        warnings.simplefilter("error")

    def __exit__(self, *a):
        return self._c.__exit__(*a)


def test_many_rejects_a_short_answer():
    with pytest.raises(RuntimeError, match="rows"):
        search_minimum_initial_balance_many(lambda rows, levels: [], 85.0, [1.0, 2.0])


def test_scenario_records_fill_defaults_and_reject_unknown_keys():
    defaults = (1000.0, 20.0, 300.0)
    assert SCENARIO_FIELDS == ("initial_balance", "monthly_contribution", "monthly_expenses")
    assert scenario_records([{}, {"monthly_expenses": 5}, {"initial_balance": 0, "monthly_contribution": 7.5, "monthly_expenses": 1}],
                            defaults) == [(1000.0, 20.0, 300.0), (1000.0, 20.0, 5.0), (0.0, 7.5, 1.0)]
    assert scenario_records([], defaults) == []
    with pytest.raises(ValueError, match=r"scenarios\[1\].*allocation_inv1_pct"):
        scenario_records([{}, {"allocation_inv1_pct": 0.5}], defaults)


def test_success_probability_by_scenarios_rejects_an_unknown_key_before_any_device_work():
    from monte_carlo_retirement_amd import Config, load_config_from_json
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    class Double(RetirementMonteCarloSimulator):   # any step towards the device fails the test
        def _current_params(self):
            raise AssertionError("device work before the key check")

        _batch_rng = _local_device = _current_params

    sim = Double(Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json"))))
    with pytest.raises(ValueError, match="retirement_years"):
        sim.success_probability_by_scenarios(0, [{"initial_balance": 1.0}, {"retirement_years": 3}], 100)
    assert sim.success_probability_by_scenarios(0, [], 100).shape == (0,)


def test_entry_point_is_exported_and_declared():
    assert "mcr_probe_scenarios_rng" in N.ABI_SYMBOLS
    assert N.MCR_ABI_VERSION == 8
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert re.search(r"#define\s+MCR_ABI_VERSION\s+8\b", header)
    assert "int mcr_probe_scenarios_rng(" in header and "const mcr_scenario* scenarios" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"typedef struct mcr_scenario \{ double initial_balance, monthly_contribution, monthly_expenses; \} mcr_scenario;", code)
    assert C.sizeof(N.McrScenario) == 24
    assert [f for f, _ in N.McrScenario._fields_] == list(SCENARIO_FIELDS)
    assert all(t is C.c_double for _, t in N.McrScenario._fields_)


def test_library_exports_the_entry_point_with_its_signature():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    lib = N.load_library()
    assert hasattr(lib, "mcr_probe_scenarios_rng")
    assert lib.mcr_probe_scenarios_rng.argtypes[6] == C.POINTER(N.McrScenario)
    assert lib.mcr_abi_version() == 8
