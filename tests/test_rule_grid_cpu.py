"""The rule-grid probe without a GPU: the two symbols and the ABI version, the host-side validation of
`mcr_probe_rule_grid_rng` (it runs before a device is looked for, and leaves both outputs untouched), the month-search driver
shared by `find_minimum_working_months` and `find_minimum_working_months_with_rule`, and the frontier under a rule on a stubbed
grid probe."""

from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
from monte_carlo_retirement_amd.spending import EXPENSE_CAP, search_maximum_expenses
from monte_carlo_retirement_amd.spending_rules import SpendingRule

import spending_rule_model as M

SYMMETRIC = M.RULES["symmetric"]
SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def lib():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    return N.load_library()


def test_header_and_binding_carry_the_symbols(lib):
    with open(os.path.join(REPO, "include", "mcr.h")) as fh:
        declared = set(re.findall(r"\b(mcr_[a-z0-9_]+)\s*\(", fh.read()))
    for sym in ("mcr_probe_rule_grid_rng", "mcr_probe_rule_grid_last_fanout_launches"):
        assert sym in declared and sym in N.ABI_SYMBOLS and hasattr(lib, sym), sym
    assert lib.mcr_abi_version() == 8 == N.MCR_ABI_VERSION
    assert lib.mcr_probe_rule_grid_last_fanout_launches() == 0


def _config(**over):
    return Config(**dict(M.plan_config("realized", REPO), **over))


class _Call:
    """One call of the entry point with HOST sentinel buffers as its outputs: validation comes before the device, so a
    refused call must leave every word of both as it was."""

    def __init__(self, lib, params, ry):
        self.lib, self.params, self.ry = lib, params, ry

    def __call__(self, rng=None, months=(120, 0, 7), levels=None, n_levels=None, rule=SYMMETRIC, n_candidates=None,
                 null=(), n_paths=64):
        months = list(months)
        n_l = 2 if levels is None else len(levels[0])
        levels = [[1000.0 + 10 * c + k for k in range(n_l)] for c in range(len(months))] if levels is None else levels
        flat = [x for row in levels for x in row]
        marr = (C.c_int32 * max(1, len(months)))(*months)
        larr = (C.c_double * max(1, len(flat)))(*flat)
        cells = max(1, len(months) * n_l)
        counts = (C.c_uint64 * (cells * N.MCR_N_COUNTERS))(*([SENTINEL] * (cells * N.MCR_N_COUNTERS)))
        years = (C.c_uint64 * (cells * self.ry * N.MCR_RULE_N_COUNTS))(*([SENTINEL] * (cells * self.ry * N.MCR_RULE_N_COUNTS)))
        rng = N.philox_rng(1) if rng is None else rng
        record = None if rule is None else N.McrSpendingRule(*rule)
        rc = self.lib.mcr_probe_rule_grid_rng(
            None if "params" in null else C.byref(self.params), None if "rng" in null else C.byref(rng), 1, 0, n_paths,
            None if "months" in null else marr, len(months) if n_candidates is None else n_candidates,
            None if "levels" in null else larr, n_l if n_levels is None else n_levels,
            None if record is None else C.byref(record), None if "counts" in null else C.addressof(counts), C.addressof(years), 0, None)
        assert all(x == SENTINEL for x in counts) and all(x == SENTINEL for x in years), "an output was written"
        assert self.lib.mcr_probe_rule_grid_last_fanout_launches() == 0
        return rc, N.last_error()


def test_validation_is_host_only_and_leaves_the_outputs_untouched(lib):
    cfg = _config()
    call = _Call(lib, params_from_config(cfg), int(cfg.retirement_years))
    # a bad month
    rc, msg = call(months=(120, -1, 7))
    assert rc == N.MCR_ERR_INVALID_ARG and "working_months" in msg, msg
    # a NaN, a negative and an infinite level: the message names the cell
    for bad, at in ((float("nan"), (1, 0)), (-1.0, (2, 1)), (float("inf"), (0, 1))):
        levels = [[1000.0, 1100.0] for _ in range(3)]
        levels[at[0]][at[1]] = bad
        rc, msg = call(levels=levels)
        assert rc == N.MCR_ERR_INVALID_ARG and msg.startswith(f"monthly_expenses[{at[0]}][{at[1]}] = "), msg
    # each out-of-range rule field
    fields = ("upper", "lower", "cut", "raise", "floor", "ceiling")
    for i, v in ((0, 0.5), (1, 1.5), (2, 1.0), (3, -0.1), (4, float("nan")), (5, 0.5)):
        rule = list(SYMMETRIC)
        rule[i] = v
        rc, msg = call(rule=rule)
        assert rc == N.MCR_ERR_INVALID_ARG and msg.startswith(f"spending rule: {fields[i]} = "), (fields[i], msg)
    # counts and pointers
    rc, msg = call(n_levels=-1)
    assert rc == N.MCR_ERR_INVALID_ARG and "n_levels" in msg, msg
    rc, msg = call(n_candidates=-1)
    assert rc == N.MCR_ERR_INVALID_ARG and "n_candidates" in msg, msg
    for which in ("months", "levels", "counts"):
        rc, msg = call(null=(which,))
        assert rc == N.MCR_ERR_INVALID_ARG and "null" in msg, (which, msg)
    rc, msg = call(rule=None)
    assert rc == N.MCR_ERR_INVALID_ARG and "null spending rule" in msg, msg
    rc, msg = call(null=("params",))
    assert rc == N.MCR_ERR_INVALID_ARG, msg
    rc, msg = call(null=("rng",))
    assert rc == N.MCR_ERR_INVALID_ARG, msg
    # an empty grid does nothing, on any box
    assert call(months=())[0] == 0 and call(n_levels=0)[0] == 0
    # what mcr_run_rule_rng refuses, by its words
    rc, msg = call(rng=N.numpy_rng(5))
    assert rc == N.MCR_ERR_UNSUPPORTED and msg == "spending rule: the NumPy stream is not supported (the engine's own stream only)", msg
    rc, msg = call(rng=N.history_rng(7, np.random.default_rng(1).standard_normal((240, 3)), 12))
    assert rc == N.MCR_ERR_UNSUPPORTED and msg == "spending rule: the history stream is not supported (the engine's own stream only)", msg
    many = dict(M.plan_config("realized", REPO))
    many["other_income_streams"] = [{"name": f"s{k}", "monthly_amount_today": 100.0 + k, "start_at_age": 50.0 + k, "duration_years": None,
                                     "inflation_indexed": True, "tax_rate": 0.1} for k in range(17)]
    cfg17 = Config(**many)
    rc, msg = _Call(lib, params_from_config(cfg17), int(cfg17.retirement_years))()
    assert rc == N.MCR_ERR_UNSUPPORTED and msg == "spending rule: 17 income streams need the generic variant (at most 16 are supported)", msg


@pytest.mark.parametrize("idx", [0, 3])
@pytest.mark.parametrize("slots", [1, 3])
def test_both_month_searches_run_the_same_driver(idx, slots):
    """`find_minimum_working_months` and `find_minimum_working_months_with_rule` on the same probability table: the same
    months, probability, curve and events; and a month the driver evaluated on speculation never reaches the curve."""
    g = load_golden("search.json")[idx]
    cfg = Config(**g["cfg"])
    n = cfg.num_simulations_search
    exact = {e["working_months"]: int(round(e["probability"] * n / 100.0)) / n * 100.0 for e in g["events"]
             if e["type"] == "search_iter"}
    known = sorted(exact)
    rule = SpendingRule(*SYMMETRIC)

    def run(with_rule: bool):
        sim = RetirementMonteCarloSimulator(cfg, main_seed_override=g["seed"])
        calls = []

        def table(months, k, *rest):
            assert k == n and len(set(months)) == len(months)
            assert rest == ((rule,) if with_rule else ())
            calls.append(list(months))
            return {m: exact.get(m, exact[min(known, key=lambda x: abs(x - m))]) for m in months}

        def must_not_run(*a, **k):
            raise AssertionError("the other search's probe ran")

        sim._probe_many = must_not_run if with_rule else table
        sim._probe_many_with_rule = table if with_rule else must_not_run
        sim._speculation_slots = lambda k: slots
        events = []
        if with_rule:
            out = sim.find_minimum_working_months_with_rule(rule, verbose=False, progress_callback=events.append)
        else:
            out = sim.find_minimum_working_months(verbose=False, progress_callback=events.append)
        return out, events, calls

    (m0, p0, c0), e0, calls0 = run(False)
    (m1, p1, c1), e1, calls1 = run(True)
    assert (m0, p0, c0, e0) == (m1, p1, c1, e1) and calls0 == calls1
    assert m0 == g["months"] and [c["working_months"] for c in c0] == [c["working_months"] for c in g["search_curve"]]
    evaluated = {m for c in calls1 for m in c}
    assert {c["working_months"] for c in c1} <= evaluated
    assert {c["working_months"] for c in c1} == set(exact)          # only what the driver asked for, speculation or not
    if slots == 1:
        assert evaluated == set(exact)


def test_probe_many_with_rule_is_one_grid_probe_with_one_level_per_row():
    cfg = _config(num_simulations_search=200)
    sim = RetirementMonteCarloSimulator(cfg, main_seed_override=5)
    rule = SpendingRule(*SYMMETRIC)
    seen = []

    def fake_grid(months, levels_2d, rule_, n):
        seen.append((list(months), [list(r) for r in levels_2d], rule_, n))
        return np.array([[50.0 + m] for m in months])

    sim._rule_grid_probabilities = fake_grid
    assert sim._probe_many_with_rule([12, 0, 24], 200, rule) == {12: 62.0, 0: 50.0, 24: 74.0}
    e0 = float(cfg.monthly_expenses)
    assert seen == [([12, 0, 24], [[e0], [e0], [e0]], rule, 200)]
    # the public grid: one column at the config's own level by default, the listed levels otherwise
    sim.success_probability_grid_with_rule([5, 6], rule, num_simulations=10)
    sim.success_probability_grid_with_rule([5], rule, [1.0, 2.0])
    assert seen[1:] == [([5, 6], [[e0], [e0]], rule, 10), ([5], [[1.0, 2.0]], rule, int(cfg.num_simulations_main))]
    with pytest.raises(ValueError, match="spending rule is required"):
        RetirementMonteCarloSimulator(cfg, main_seed_override=5)._rule_grid_probabilities([1], [[1.0]], None, 10)


def test_frontier_under_a_rule_equals_the_single_searches_on_a_stub_curve():
    """`find_maximum_initial_expenses_by_months` on a stubbed grid probe: per month what `search_maximum_expenses` returns on
    the same curve, and every round is one call of the grid."""
    cfg = _config(num_simulations_search=500, target_probability=90.0)
    sim = RetirementMonteCarloSimulator(cfg, main_seed_override=5)
    rule = SpendingRule(*SYMMETRIC)
    months = [0, 120, 240]

    def curve(month, level):                      # falls with the level, rises with the month; crosses 90 % at a month's own level
        return max(0.0, min(100.0, 100.0 - 10.0 * level / (1500.0 + 20.0 * month)))

    rounds = []

    def fake_grid(ms, levels_2d, rule_, n):
        assert rule_ is rule and n == 500
        rounds.append(list(ms))
        return np.array([[curve(m, x) for x in row] for m, row in zip(ms, levels_2d)])

    sim._rule_grid_probabilities = fake_grid
    events = []
    got = sim.find_maximum_initial_expenses_by_months(months, rule, verbose=False, progress_callback=events.append)
    start = max(float(cfg.monthly_expenses), 1.0)
    for m, (expenses, prob, c) in zip(months, got):
        want = search_maximum_expenses(lambda levels, m=m: [curve(m, x) for x in levels], 90.0, start,
                                       levels_per_call=N.MCR_MAX_EXPENSE_FANOUT, resolution=1.0, cap=EXPENSE_CAP)
        assert (expenses, prob, c) == tuple(want), m
        assert 0.0 <= (1500.0 + 20.0 * m) - expenses <= 1.0       # (the curve's crossing, to the search's resolution)
    assert rounds and all(set(r) <= set(months) for r in rounds) and rounds[0] == months
    assert {e["working_months"] for e in events} == set(months)
