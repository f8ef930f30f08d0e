"""Scenario and assumption options for the stratified random plans of tests/count_fuzz.py, with the CPU oracle's answer to each.

The outcome and joint probes of the scenario and assumption families are compared elsewhere with the library's own launches.
Here every option is a `Config` override the ORACLE can run, so its per-path columns are the reference
(tests/test_gpu_probe_options_vs_oracle.py), and tests/test_option_fuzz_cpu.py shows from the oracle alone that the options
are worth running: they move paths, and they leave most plans with both outcomes.

Scenario options of a plan (initial_balance, monthly_contribution, monthly_expenses):
    own:  the plan's own triple
    A:    (initial_balance, 0.5 x contribution, 1.05 x expenses)
    B:    (1.25 x initial_balance, contribution, 0.9 x expenses)
Assumption options: the plan's own record, and the market record of tests/test_gpu_count_routes_vs_oracle.py
(inv1_returns_mean - 0.02, rho moved by 0.3).

(The harsher pair of that test, 1.25 x expenses with 0.5 x contribution, leaves 22 of the 68 plans with mixed outcomes: too few
successes for the final-balance rows.)"""

from __future__ import annotations

import numpy as np

import count_fuzz as F

FAMILIES = ("scenarios", "assumptions")
SCENARIO_FIELDS = ("initial_balance", "monthly_contribution", "monthly_expenses")
NAMES = {"scenarios": ("own", "A", "B"), "assumptions": ("own", "market")}


def moved_rho(rho):
    return rho + 0.3 if rho + 0.3 <= 1.0 else rho - 0.3


def overrides(scn, family):
    """The `Config` fields each option of `family` replaces: one dict per option, {} for the plan's own."""
    c = scn.cfgd
    if family == "scenarios":
        return [{}, dict(monthly_contribution=0.5 * c["monthly_contribution"], monthly_expenses=1.05 * c["monthly_expenses"]),
                dict(initial_balance=1.25 * c["initial_balance"], monthly_expenses=0.9 * c["monthly_expenses"])]
    assert family == "assumptions", family
    return [{}, {"inv1_returns_mean": c["inv1_returns_mean"] - 0.02, "equity_inflation_correlation": moved_rho(c["equity_inflation_correlation"])}]


def triples(scn):
    """The scenario options as the probe takes them."""
    return [tuple(float(dict(scn.cfgd, **o)[f]) for f in SCENARIO_FIELDS) for o in overrides(scn, "scenarios")]


def class_runs(O, cls, family):
    """[(plan, [the oracle's trajectory run of each option])] of class `cls`: on host threads, cached by count_fuzz."""
    plans = F.scenarios(O, cls)
    jobs = [((scn,), dict(trajectories=True, **o)) for scn in plans for o in overrides(scn, family)]
    runs = F.oracle_runs(O, jobs)
    n = len(NAMES[family])
    return [(scn, runs[n * k: n * k + n]) for k, scn in enumerate(plans)]


def oracle_rows(runs):
    """(final_balance where the path succeeds else NaN, years_to_ruin, the path's money scale), [options, n] each."""
    fin = np.stack([np.where(np.asarray(r["success"]).astype(bool), r["final_balance"], np.nan) for r in runs])
    ruin = np.stack([np.asarray(r["years_to_ruin"], dtype=np.float64) for r in runs])
    scale = np.stack([np.maximum(1.0, np.abs(r["trajectory"]).max(axis=0)) for r in runs])
    return fin, ruin, scale


def oracle_flags(runs):
    return np.stack([np.asarray(r["success"]).astype(np.uint8) for r in runs])
