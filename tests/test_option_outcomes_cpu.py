"""`outcomes.OptionOutcomes` on hand-made tables, the validation of the `option_outcomes_by_*` methods, and the claim / stress
documents with and without ``outcomes=True`` -- no GPU: the probes are stubbed as in the `*_search_cpu` tests."""

from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.income import INCOME_OPTION_FIELDS
from monte_carlo_retirement_amd.outcomes import CONFIDENCE_LEVELS, DEFAULT_QUANTILES, OptionOutcomes, quantile_key
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

RY = 2                      # a two-year horizon: months 0 .. 24
CELLS = 12 * RY + 1
QS = DEFAULT_QUANTILES
AGE = 60.0


def table(*rows):
    """Ruin tables from {month: paths} dicts."""
    out = np.zeros((len(rows), CELLS), dtype=np.int64)
    for k, row in enumerate(rows):
        for m, c in row.items():
            out[k, m] = c
    return out


def outcomes(n, *rows, quantiles=None):
    months = table(*rows)
    successes = n - months.sum(axis=1)
    fq = np.array([[1000.0 * (k + 1) + 100.0 * j for j in range(len(QS))] for k in range(len(rows))]) if quantiles is None else quantiles
    return OptionOutcomes(successes, n, months, QS, fq, successes, AGE)


def test_no_failures():
    o = outcomes(100, {})
    assert o.probabilities.tolist() == [100.0] and o.failures(0) == 0
    assert o.ruined_by(0).tolist() == [0.0] * CELLS
    assert all(o.lasts_months(0, c) is None and o.lasts_until_age(0, c) is None for c in (0.5, 0.9, 0.99, 1.0))
    assert o.median_ruin_age(0) is None
    assert o.final_balance(0) == {q: 1000.0 + 100.0 * j for j, q in enumerate(QS)}
    assert o.row(0)["lasts_until_age"] == {"90": None, "95": None, "99": None} and o.row(0)["median_ruin_age"] is None


def test_all_failures_and_the_empty_cohort():
    o = outcomes(100, {3: 50, 10: 50}, quantiles=np.full((1, len(QS)), np.nan))
    assert o.probabilities.tolist() == [0.0] and o.cohort.tolist() == [0]
    assert o.final_balance(0) == {q: None for q in QS}                       # None, never a made-up 0.0
    assert o.row(0)["final_balance"] == {"p5": None, "p25": None, "p50": None, "p75": None, "p95": None}
    assert o.lasts_months(0, 0.95) == 2 and o.lasts_months(0, 0.5) == 9 and o.lasts_months(0, 0.49) == 9
    assert o.lasts_months(0, 1.0) == 2                                       # no path may fail: month 2 is the last clean one
    assert o.median_ruin_age(0) == AGE + (3 + 10) / 2.0 / 12.0               # 100 failures: the mean of ranks 49 and 50
    assert o.ruined_by(0)[[2, 3, 9, 10, 24]].tolist() == [0.0, 0.5, 0.5, 1.0, 1.0]


def test_every_failure_in_month_zero():
    o = outcomes(100, {0: 20})
    assert o.probabilities.tolist() == [80.0]
    assert o.lasts_months(0, 0.95) == -1 and o.lasts_until_age(0, 0.95) == AGE     # fails that confidence before retirement
    assert o.lasts_months(0, 0.8) is None                                    # exactly on the step: 20 of 100 is allowed at 80 %
    assert o.lasts_months(0, 0.81) == -1
    assert o.median_ruin_age(0) == AGE
    assert o.ruined_by(0).tolist() == [0.2] * CELLS


def test_every_failure_in_the_last_month():
    o = outcomes(1000, {24: 100})
    assert o.lasts_months(0, 0.95) == 23 and o.lasts_until_age(0, 0.95) == AGE + 23 / 12.0
    assert o.lasts_months(0, 0.9) is None and o.lasts_months(0, 0.85) is None
    assert o.lasts_months(0, 0.901) == 23
    assert o.median_ruin_age(0) == AGE + 2.0


def test_confidence_exactly_on_a_cumulative_step():
    # cumulative shares: 1 % after month 5, 5 % after month 7, 10 % after month 12, 10.1 % after month 20
    o = outcomes(1000, {5: 10, 7: 40, 12: 50, 20: 1})
    assert o.lasts_months(0, 0.99) == 6          # 1 % is allowed through month 6; month 7 brings 5 %
    assert o.lasts_months(0, 0.95) == 11         # exactly 5 % through month 11
    assert o.lasts_months(0, 0.9) == 19          # exactly 10 % through month 19
    assert o.lasts_months(0, 0.899) is None      # 10.1 % allowed: the whole horizon
    assert o.lasts_months(0, 0.991) == 4 and o.lasts_months(0, 0.951) == 6 and o.lasts_months(0, 0.949) == 11
    assert o.lasts_months(0, 0.3) is None
    # odd count: the median is the middle failure's month (0-based rank 50 of 101; ranks 50 .. 99 fail in month 12)
    assert o.median_ruin_age(0) == AGE + 1.0
    assert outcomes(1000, {5: 10, 7: 41, 12: 50}).median_ruin_age(0) == AGE + 7 / 12.0       # rank 50 is the last of month 7
    with pytest.raises(ValueError):
        o.lasts_months(0, 0.0)
    with pytest.raises(ValueError):
        o.lasts_months(0, 1.5)


def test_probabilities_are_the_plain_probes_percentages():
    n = 7919
    o = outcomes(n, {1: 1234}, {2: 7919}, {})
    want = [RetirementMonteCarloSimulator._count_percent(c, n) for c in (n - 1234, 0, n)]
    assert o.probabilities.tolist() == want and o.probabilities.dtype == np.float64
    assert len(o) == 3 and o.horizon_months == 24


def test_constructor_checks_and_equality():
    with pytest.raises(ValueError):
        OptionOutcomes([5], 10, np.zeros((1, 24)), QS, np.zeros((1, 5)), [5], AGE)          # 24 cells is no 12 ry + 1
    with pytest.raises(ValueError):
        OptionOutcomes([9], 10, table({1: 2}), QS, np.zeros((1, 5)), [9], AGE)             # 11 paths of 10
    with pytest.raises(ValueError):
        OptionOutcomes([5], 10, table({1: 5}), QS, np.zeros((1, 5)), [5, 5], AGE)
    a, b = outcomes(100, {3: 5}), outcomes(100, {3: 5})
    assert a == b and not (a != b) and a != outcomes(100, {4: 5})
    empty = OptionOutcomes([], 100, np.zeros((0, CELLS)), QS, np.zeros((0, 5)), [], AGE)
    assert len(empty) == 0 and empty.probabilities.tolist() == []
    assert quantile_key(0.05) == "p5" and quantile_key(0.5) == "p50" and quantile_key(0.975) == "p97.5"
    assert CONFIDENCE_LEVELS == (0.90, 0.95, 0.99)


# ---- the simulator: validation before any device work, documents -----------------------------------------------------------
def _simulator():
    return RetirementMonteCarloSimulator(Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json"))))


OPTIONS = [{"start_at_age": 62.0, "monthly_amount_today": 1400.0}, {"start_at_age": 67.0, "monthly_amount_today": 2000.0},
           {"start_at_age": 70.0, "monthly_amount_today": 2480.0}]


def test_option_validation_raises_before_any_device_work(monkeypatch):
    sim = _simulator()
    for name in ("probe_scenarios_outcomes", "probe_income_outcomes", "probe_assumptions_outcomes", "ruin_month_counts"):
        monkeypatch.setattr(E, name, lambda *a, **k: pytest.fail("validation comes before the device"))
    with pytest.raises(ValueError):
        sim.option_outcomes_by_scenarios(240, [{"monthly_expences": 1.0}], 100)
    with pytest.raises(ValueError):
        sim.option_outcomes_by_income_options(240, "No Such Stream", OPTIONS, 100)
    with pytest.raises(ValueError):
        sim.option_outcomes_by_income_options(240, 0, [{"claim_age": 62.0}], 100)
    with pytest.raises(ValueError):
        sim.option_outcomes_by_assumptions(240, [{"inv1_returns_meen": 0.1}], 100)
    with pytest.raises(ValueError):
        sim.option_outcomes_by_scenarios(240, [{}], 100, quantiles=(0.5, 1.5))
    empty = sim.option_outcomes_by_scenarios(240, [], 100)                    # no option: no device either
    assert len(empty) == 0 and empty.n_paths == 100 and empty.horizon_months == 12 * sim.params_model.retirement_years


def _three(n=1000):
    ry = 50
    months = np.zeros((3, 12 * ry + 1), dtype=np.int64)
    months[0, [100, 200]] = [300, 100]
    months[1, 300] = 245
    successes = n - months.sum(axis=1)
    fq = np.array([[1e5, 2e5, 3e5, 4e5, 5e5], [2e5, 3e5, 4e5, 5e5, 6e5], [3e5, 4e5, 5e5, 6e5, 7e5]])
    return OptionOutcomes(successes, n, months, QS, fq, successes, 60.0)


def test_claiming_document_is_unchanged_without_outcomes(monkeypatch):
    sim = _simulator()
    monkeypatch.setattr(sim, "success_probability_by_income_options", lambda wm, s, o, n=None: np.array([60.0, 75.5, 75.5]))
    monkeypatch.setattr(sim, "option_outcomes_by_income_options", lambda *a, **k: pytest.fail("outcomes=False must not run the outcomes probe"))
    docs = [sim.compare_claiming_options(240, 0, OPTIONS, 1000), sim.compare_claiming_options(240, 0, OPTIONS, 1000, outcomes=False),
            sim.compare_claiming_options(240, 0, OPTIONS, 1000, paired=False, outcomes=False)]
    for doc in docs:
        assert list(doc) == ["stream", "options", "best"] and doc["best"] == 1 and doc["stream"] == 0
        assert all(list(r) == list(INCOME_OPTION_FIELDS) + ["probability"] for r in doc["options"])
    assert docs[0] == docs[1] == docs[2]


def test_claiming_document_with_outcomes(monkeypatch):
    sim = _simulator()
    O = _three()
    monkeypatch.setattr(sim, "option_outcomes_by_income_options", lambda wm, s, o, n=None: O)
    monkeypatch.setattr(sim, "success_probability_by_income_options", lambda *a, **k: pytest.fail("one probe serves outcomes=True"))
    doc = sim.compare_claiming_options(240, 0, OPTIONS, 1000, outcomes=True)
    assert list(doc) == ["stream", "options", "best"] and doc["best"] == 2
    assert [r["probability"] for r in doc["options"]] == O.probabilities.tolist() == [60.0, 75.5, 100.0]
    assert all(list(r) == list(INCOME_OPTION_FIELDS) + ["probability", "lasts_until_age", "median_ruin_age", "final_balance"] for r in doc["options"])
    a, b, c = doc["options"]
    assert a["lasts_until_age"] == {"90": 60.0 + 99 / 12.0, "95": 60.0 + 99 / 12.0, "99": 60.0 + 99 / 12.0}
    assert a["median_ruin_age"] == 60.0 + 100 / 12.0 and b["median_ruin_age"] == 85.0 and c["median_ruin_age"] is None
    assert b["lasts_until_age"]["90"] == 60.0 + 299 / 12.0 and c["lasts_until_age"] == {"90": None, "95": None, "99": None}
    assert a["final_balance"] == {"p5": 1e5, "p25": 2e5, "p50": 3e5, "p75": 4e5, "p95": 5e5}


def test_stress_table_with_and_without_outcomes(monkeypatch):
    sim = _simulator()
    shifts = [("equity -1", {"inv1_returns_mean": -0.01}), ("inflation +1", {"inflation_rate_mean": 0.01})]
    monkeypatch.setattr(sim, "success_probability_by_assumptions", lambda wm, s, n=None: np.array([80.0, 70.0, 78.0]))
    monkeypatch.setattr(sim, "option_outcomes_by_assumptions", lambda *a, **k: pytest.fail("outcomes=False must not run the outcomes probe"))
    plain = [sim.stress_test(240, shifts, 1000), sim.stress_test(240, shifts, 1000, outcomes=False)]
    for t in plain:
        assert len(t) == 3 and all(list(r) == ["label", "overrides", "probability", "delta"] for r in t)
        assert [r["delta"] for r in t] == [0.0, -10.0, -2.0]
    assert plain[0] == plain[1]
    O = _three()
    monkeypatch.setattr(sim, "option_outcomes_by_assumptions", lambda wm, s, n=None: O)
    monkeypatch.setattr(sim, "success_probability_by_assumptions", lambda *a, **k: pytest.fail("one probe serves outcomes=True"))
    rich = sim.stress_test(240, shifts, 1000, outcomes=True)
    assert all(list(r) == ["label", "overrides", "probability", "delta", "lasts_until_age", "median_ruin_age", "final_balance"] for r in rich)
    assert [r["probability"] for r in rich] == [60.0, 75.5, 100.0] and [r["delta"] for r in rich] == [0.0, 15.5, 40.0]
    assert [{k: r[k] for k in ("lasts_until_age", "median_ruin_age", "final_balance")} for r in rich] == [O.row(k) for k in range(3)]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    return N.load_library()


OUTCOME_SYMBOLS = ("mcr_probe_scenarios_outcomes_rng", "mcr_probe_assumptions_outcomes_rng", "mcr_probe_income_outcomes_rng",
                   "mcr_ruin_month_counts")


def test_header_declares_and_native_binds_the_outcome_entries(lib):
    hdr = open(os.path.join(REPO, "include", "mcr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef struct mcr_option_outcomes \{\s*double\* final_balance;\s*double\* years_to_ruin;\s*int64_t path_stride;\s*\} mcr_option_outcomes;", code)
    for sym in OUTCOME_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", code), sym
        assert sym in N.ABI_SYMBOLS and hasattr(lib, sym), sym
    assert C.sizeof(N.McrOptionOutcomes) == 24
    assert len(lib.mcr_probe_income_outcomes_rng.argtypes) == len(lib.mcr_probe_income_rng.argtypes) + 1
    assert len(lib.mcr_probe_scenarios_outcomes_rng.argtypes) == len(lib.mcr_probe_scenarios_rng.argtypes) + 1
    assert len(lib.mcr_probe_assumptions_outcomes_rng.argtypes) == len(lib.mcr_probe_assumptions_rng.argtypes) + 1


def test_invalid_outcome_arguments_return_before_any_device_call(lib):
    """A short path_stride and the reduction's argument checks answer MCR_ERR_INVALID_ARG (-1) with or without a GPU, never
    MCR_ERR_NO_DEVICE, and no pointer is touched (they are small integers here)."""
    p = params_from_config(Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json"))))
    rng = N.McrRng()
    rng.kind, rng.philox_seed = N.MCR_RNG_PHILOX, 1
    head = (C.byref(p), C.byref(rng), 0, 0, 1000, 12)
    fake = C.c_void_p(8)
    rows = N.McrOptionOutcomes(8, 8, 999)
    sc, am, io = (N.McrScenario * 3)(), (N.McrAssumptions * 3)(), (N.McrIncomeOption * 3)()
    assert lib.mcr_probe_scenarios_outcomes_rng(*head, sc, 3, fake, C.byref(rows), 0, None) == -1 and "path_stride 999 < n_paths 1000" in N.last_error()
    assert lib.mcr_probe_assumptions_outcomes_rng(*head, am, 3, fake, C.byref(rows), 0, None) == -1 and "path_stride" in N.last_error()
    assert lib.mcr_probe_income_outcomes_rng(*head, 0, io, 3, fake, C.byref(rows), 0, None) == -1 and "path_stride" in N.last_error()
    for args in ((fake, 999, 2, 1000, 30, fake), (fake, 1000, -1, 1000, 30, fake), (fake, 1000, 2, -1, 30, fake), (fake, 1000, 2, 1000, 0, fake)):
        assert lib.mcr_ruin_month_counts(*args, 0, None) == -1, args
    assert lib.mcr_ruin_month_counts(None, 1000, 0, 1000, 30, None, 0, None) == 0          # no rows: nothing to do
    assert lib.mcr_ruin_month_counts(None, 0, 3, 0, 30, None, 0, None) == 0                # no paths: nothing to do
