"""`stress.py` without a GPU: the assumption records, the default stress table, the break-even search on synthetic probes, and the
header / binding agreement on `mcr_probe_assumptions_rng`."""

from __future__ import annotations

import ctypes as C
import logging
import math
import os
import re
import warnings

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.stress import (ADVERSE_DIRECTION, ASSUMPTION_FIELDS, DEFAULT_SHIFTS, MARKET_FIELDS, assumption_records,
                                               field_bounds, search_breakeven, stress_scenarios)

RECORD_FIELDS = ("initial_balance", "monthly_contribution", "monthly_expenses", "inv1_mu_log", "inv1_sigma_log", "inf_mu_log",
                 "inf_sigma_log", "prem_mu_log", "prem_sigma_log", "equity_inflation_rho")


def _config(**over):
    return Config(**dict(load_config_from_json(os.path.join(REPO, "scenarios", "config.json")), **over))


def _record_of(cfg):
    p = params_from_config(cfg)
    return tuple(float(getattr(p, f)) for f in RECORD_FIELDS)


# ---- assumption_records ----------------------------------------------------------------------------
def test_fields():
    assert MARKET_FIELDS == ("inv1_returns_mean", "inv1_returns_volatility", "inflation_rate_mean", "inflation_rate_volatility",
                             "inv2_premium_over_inflation_mean", "inv2_premium_over_inflation_volatility",
                             "equity_inflation_correlation")
    assert ASSUMPTION_FIELDS == MARKET_FIELDS + ("initial_balance", "monthly_contribution", "monthly_expenses")
    assert all(f in Config.model_fields for f in ASSUMPTION_FIELDS)
    assert set(ADVERSE_DIRECTION) == set(MARKET_FIELDS) - {"equity_inflation_correlation"}


def test_records_take_defaults_and_equal_params_from_config():
    cfg = _config()
    overrides = [{}, {"inv1_returns_mean": 0.03}, {"inv1_returns_volatility": 0.0, "inflation_rate_volatility": 0.0,
                                                   "inv2_premium_over_inflation_volatility": 0.0},
                 {"equity_inflation_correlation": -1.0, "inflation_rate_mean": 0.3, "monthly_expenses": 1234.5},
                 {f: v for f, v in zip(ASSUMPTION_FIELDS, (-0.4, 0.9, 0.07, 0.03, -0.02, 0.11, 0.5, 1.0, 2.0, 3.0))}]
    got = assumption_records(cfg, overrides)
    assert got[0] == _record_of(cfg)
    for o, r in zip(overrides, got):
        assert r == _record_of(_config(**o)), o        # the same bits as the modified Config's parameter block
        assert len(r) == 10 and all(isinstance(x, float) for x in r)
    assert assumption_records(cfg, []) == []


def test_records_reject_unknown_keys_and_out_of_bounds_values():
    cfg = _config()
    with pytest.raises(ValueError, match=r"scenarios\[1\].*allocation_inv1_pct"):
        assumption_records(cfg, [{}, {"allocation_inv1_pct": 0.5}])
    for bad in ({"inv1_returns_volatility": -0.01}, {"equity_inflation_correlation": 1.5}, {"inflation_rate_mean": -1.0},
                {"initial_balance": -1.0}, {"inv1_returns_mean": float("nan")}):
        with pytest.raises(ValueError, match=r"scenarios\[2\]"):
            assumption_records(cfg, [{}, {}, bad])


def test_record_validation_keeps_the_soft_volatility_warnings_silent():
    """`Config` warns about a low equity or a high inflation volatility whenever one is built; the records of a probe (a
    volatility search: every level) are validated by building one and must not repeat it."""
    from monte_carlo_retirement_amd._logging import logger

    seen = []
    if isinstance(logger, logging.Logger):
        handler = logging.Handler()
        handler.emit = lambda record: seen.append(record.getMessage())
        logger.addHandler(handler)
        remove = lambda: logger.removeHandler(handler)
    else:
        sink = logger.add(lambda message: seen.append(str(message)))
        remove = lambda: logger.remove(sink)
    try:
        cfg = _config()
        _config(inv1_returns_volatility=0.01)
        n = len(seen)
        assert n >= 1                                    # (the handler does see the warning of a Config built directly)
        got = assumption_records(cfg, [{}] + [{"inv1_returns_volatility": 0.005 * k} for k in range(8)] + [{"inflation_rate_volatility": 0.2}])
        assert len(got) == 10 and len(seen) == n
        _config(inflation_rate_volatility=0.2)
        assert len(seen) > n and "Inflation volatility (20.0%)" in seen[-1]      # (and the logger is as it was afterwards)
    finally:
        remove()


def test_class_method_rejects_bad_records_before_any_device_work():
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    class Double(RetirementMonteCarloSimulator):   # any step towards the device fails the test
        def _current_params(self):
            raise AssertionError("device work before the record check")

        _batch_rng = _local_device = _current_params

    sim = Double(_config())
    with pytest.raises(ValueError, match=r"scenarios\[1\].*retirement_years"):
        sim.success_probability_by_assumptions(0, [{"inv1_returns_mean": 0.01}, {"retirement_years": 3}], 100)
    with pytest.raises(ValueError, match=r"scenarios\[0\]"):
        sim.success_probability_by_assumptions(0, [{"inflation_rate_volatility": -0.5}], 100)
    assert sim.success_probability_by_assumptions(0, [], 100).shape == (0,)


# ---- the stress table --------------------------------------------------------------------------------
def test_default_stress_table():
    cfg = _config()
    rows = stress_scenarios(cfg)
    assert len(rows) == 15 and rows[0] == ("base", {})
    assert [label for label, _ in rows[1:]] == [label for label, _ in DEFAULT_SHIFTS]
    assert len({label for label, _ in rows}) == 15
    want = [("inv1_returns_mean", -0.02), ("inv1_returns_mean", -0.01), ("inv1_returns_mean", 0.01),
            ("inv1_returns_volatility", 0.05), ("inv1_returns_volatility", -0.05),
            ("inflation_rate_mean", 0.02), ("inflation_rate_mean", 0.01), ("inflation_rate_mean", -0.01),
            ("inflation_rate_volatility", 0.01),
            ("inv2_premium_over_inflation_mean", -0.01), ("inv2_premium_over_inflation_mean", 0.01),
            ("inv2_premium_over_inflation_volatility", 0.02),
            ("equity_inflation_correlation", -0.3), ("equity_inflation_correlation", 0.3)]
    for (label, o), (field, delta) in zip(rows[1:], want):
        lo, hi = field_bounds(field)
        assert o == {field: min(max(getattr(cfg, field) + delta, lo), hi)}, label
    assumption_records(cfg, [o for _, o in rows])      # every row is a valid record


def test_stress_table_clips_to_the_config_bounds():
    cfg = _config(inv1_returns_volatility=0.02, equity_inflation_correlation=0.9, inflation_rate_mean=-0.985)
    rows = dict(stress_scenarios(cfg))
    assert rows["equity vol -5 pts"] == {"inv1_returns_volatility": 0.0}
    assert rows["correlation +0.3"] == {"equity_inflation_correlation": 1.0}
    assert rows["inflation mean -1 pt"] == {"inflation_rate_mean": -0.99}
    assert rows["equity vol +5 pts"] == {"inv1_returns_volatility": pytest.approx(0.07)}


def test_custom_shifts_and_combined_rows():
    cfg = _config()
    rows = stress_scenarios(cfg, [("stagflation", {"inv1_returns_mean": -0.02, "inflation_rate_mean": 0.02}), ("lean", {"monthly_expenses": -500.0})])
    assert [label for label, _ in rows] == ["base", "stagflation", "lean"]
    assert rows[1][1] == {"inv1_returns_mean": cfg.inv1_returns_mean - 0.02, "inflation_rate_mean": cfg.inflation_rate_mean + 0.02}
    assert rows[2][1] == {"monthly_expenses": cfg.monthly_expenses - 500.0}
    with pytest.raises(ValueError, match=r"shifts\[0\].*retirement_years"):
        stress_scenarios(cfg, [("x", {"retirement_years": 1})])


# ---- the break-even search ----------------------------------------------------------------------------
RES = 1e-4


def _k(v):
    return round(v / RES)


def _step_probe(field, threshold_k, calls=None):
    """hits exactly on the favourable side of level threshold_k (inclusive)"""
    d = ADVERSE_DIRECTION[field]

    def probe(values):
        if calls is not None:
            calls.append(list(values))
        return [90.0 if (_k(v) >= threshold_k if d < 0 else _k(v) <= threshold_k) else 10.0 for v in values]
    return probe


def _bound(window, resolution=RES):
    return 1 + math.ceil(math.log(2 * window / resolution) / math.log(16) - 1e-12)


@pytest.mark.parametrize("field,base,threshold", [
    ("inv1_returns_mean", 0.07, 0.0312), ("inv1_returns_mean", 0.07, -0.1799), ("inv2_premium_over_inflation_mean", 0.01, 0.0099),
    ("inflation_rate_mean", 0.02, 0.0551), ("inflation_rate_mean", 0.02, 0.2699), ("inv1_returns_volatility", 0.15, 0.2203),
    ("inflation_rate_volatility", 0.01, 0.0101), ("inv2_premium_over_inflation_volatility", 0.02, 0.0007)])
def test_step_is_found_exactly_in_both_directions(field, base, threshold):
    calls, events = [], []
    value, prob, curve, status = search_breakeven(_step_probe(field, _k(threshold), calls), 85.0, field, base, on_level=events.append)
    assert status == "found" and value == pytest.approx(threshold, abs=1e-12) and prob == 90.0
    assert len(calls) <= _bound(0.25)
    assert all(len(c) <= 15 and len(set(c)) == len(c) for c in calls)
    lo_b, hi_b = field_bounds(field)
    for c in curve:      # multiples of the resolution, inside the clipped window
        assert abs(c["value"] / RES - round(c["value"] / RES)) < 1e-6
        assert max(lo_b, base - 0.25) - 1e-9 <= c["value"] <= min(hi_b, base + 0.25) + 1e-9
    assert len(curve) == len(events) == sum(len(c) for c in calls)
    assert {e["type"] for e in events} == {"breakeven_search_iter"} and {e["field"] for e in events} == {field}
    assert [e["iteration"] for e in events] == sorted(e["iteration"] for e in events)
    # the first call: both ends of the window and 13 interior levels
    assert len(calls[0]) == 15
    assert min(calls[0]) == pytest.approx(max(lo_b, base - 0.25), abs=RES) and max(calls[0]) == pytest.approx(min(hi_b, base + 0.25), abs=RES)


def test_smooth_monotone_probe_keeps_the_invariant():
    def probe(values):
        return [100.0 / (1.0 + math.exp(-(v - 0.04) * 80.0)) for v in values]
    value, prob, curve, status = search_breakeven(probe, 85.0, "inv1_returns_mean", 0.07)
    seen = {round(c["value"], 10): c["probability"] for c in curve}
    assert status == "found" and seen[round(value, 10)] == prob >= 85.0 > seen[round(value - RES, 10)]
    assert probe([value])[0] >= 85.0 > probe([value - RES])[0]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("field", ["inv1_returns_mean", "inflation_rate_mean"])
def test_noisy_non_monotone_keeps_the_invariant(seed, field):
    d = ADVERSE_DIRECTION[field]
    noise = np.random.default_rng(seed)
    memo = {}

    def probe(values):
        out = []
        for v in values:
            k = _k(v)
            if k not in memo:
                memo[k] = 85.0 - d * (v - 0.05) * 400.0 + noise.normal(0.0, 1.5)
            out.append(memo[k])
        return out
    calls = []
    value, prob, curve, status = search_breakeven(lambda vs: (calls.append(1), probe(vs))[1], 85.0, field, 0.06)
    assert status == "found" and len(calls) <= _bound(0.25)
    seen = {_k(c["value"]): c["probability"] for c in curve}
    assert seen[_k(value)] == prob >= 85.0 > seen[_k(value) + d]     # the neighbour on the adverse side was evaluated and misses


def test_always_hit_holds_at_the_adverse_window_end():
    calls = []
    for field, base, end in (("inv1_returns_mean", 0.07, -0.18), ("inflation_rate_mean", 0.02, 0.27), ("inv1_returns_volatility", 0.15, 0.40)):
        value, prob, curve, status = search_breakeven(lambda vs: (calls.append(1), [99.0] * len(vs))[1], 85.0, field, base)
        assert status == "holds_at_window_end" and value == pytest.approx(end, abs=1e-12) and prob == 99.0 and len(curve) == 15
    assert len(calls) == 3


def test_never_hit_warns_and_returns_none():
    with pytest.warns(RuntimeWarning, match="inv1_returns_mean"):
        value, prob, curve, status = search_breakeven(lambda vs: [float(_k(v) % 7) for v in vs], 85.0, "inv1_returns_mean", 0.07)
    assert value is None and status == "not_reached" and len(curve) == 15
    assert prob == float(_k(0.32) % 7)       # the favourable end's


def test_window_is_clipped_to_the_config_bounds():
    calls = []
    value, _, curve, status = search_breakeven(_step_probe("inv1_returns_volatility", _k(0.0), calls), 85.0, "inv1_returns_volatility", 0.02,
                                               window=0.25)
    assert status == "found" and value == 0.0            # only a volatility of exactly 0 hits: the clipped favourable end
    assert min(c["value"] for c in curve) == 0.0 and max(c["value"] for c in curve) == pytest.approx(0.27)
    value, _, curve, status = search_breakeven(lambda vs: [99.0] * len(vs), 85.0, "inv1_returns_mean", -0.9, window=0.25)
    assert status == "holds_at_window_end" and value == pytest.approx(-0.99)      # means stop at -0.99
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        value, _, curve, status = search_breakeven(_step_probe("inflation_rate_mean", _k(-0.9), None), 85.0, "inflation_rate_mean", -0.95, window=0.1)
    assert status == "found" and value == pytest.approx(-0.9) and min(c["value"] for c in curve) == pytest.approx(-0.99)


@pytest.mark.parametrize("window,resolution", [(0.25, 1e-4), (0.1, 1e-4), (0.25, 1e-3), (0.05, 1e-5), (0.003, 1e-4)])
def test_call_count_bound(window, resolution):
    worst = 0
    span = round(2 * window / resolution)
    base_k = round(0.5 / resolution)
    for th in sorted({1, 2, span // 14, span // 14 + 1, span // 3, span // 2, span - 2, span - 1}):
        calls = []

        def probe(values):
            calls.append(1)
            return [90.0 if round(v / resolution) >= base_k - span // 2 + th else 10.0 for v in values]
        value, _, _, status = search_breakeven(probe, 85.0, "inv1_returns_mean", 0.5, window=window, resolution=resolution)
        assert status == "found" and round(value / resolution) == base_k - span // 2 + th
        worst = max(worst, len(calls))
    assert worst <= _bound(window, resolution)


def test_argument_checks():
    ok = lambda vs: [0.0] * len(vs)     # noqa: E731
    with pytest.raises(ValueError, match="equity_inflation_correlation"):
        search_breakeven(ok, 85.0, "equity_inflation_correlation", 0.0)
    with pytest.raises(ValueError, match="monthly_expenses"):
        search_breakeven(ok, 85.0, "monthly_expenses", 100.0)
    with pytest.raises(ValueError):
        search_breakeven(ok, 85.0, "inv1_returns_mean", 0.07, resolution=0.0)
    with pytest.raises(ValueError):
        search_breakeven(ok, 85.0, "inv1_returns_mean", 0.07, window=-1.0)
    with pytest.raises(RuntimeError, match="returned 0 values"):
        search_breakeven(lambda vs: [], 85.0, "inv1_returns_mean", 0.07)


# ---- header and binding ---------------------------------------------------------------------------------
def test_entry_point_is_exported_and_declared():
    assert "mcr_probe_assumptions_rng" in N.ABI_SYMBOLS and "mcr_probe_assumptions_last_fanout_launches" in N.ABI_SYMBOLS
    assert N.MCR_ABI_VERSION == 8
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert re.search(r"#define\s+MCR_ABI_VERSION\s+8\b", header)
    assert "int mcr_probe_assumptions_rng(" in header and "const mcr_assumptions* records" in header
    assert "int mcr_probe_assumptions_last_fanout_launches(void);" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"typedef struct mcr_assumptions \{(.*?)\} mcr_assumptions;", code, flags=re.S)
    assert m
    names = [n.strip() for decl in m.group(1).split(";") if decl.strip() for n in decl.replace("double", "").split(",")]
    assert names == list(RECORD_FIELDS)
    assert C.sizeof(N.McrAssumptions) == 80
    assert [f for f, _ in N.McrAssumptions._fields_] == list(RECORD_FIELDS)
    assert all(t is C.c_double for _, t in N.McrAssumptions._fields_)


def test_library_exports_the_entry_point_with_its_signature():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    lib = N.load_library()
    assert hasattr(lib, "mcr_probe_assumptions_rng")
    assert lib.mcr_probe_assumptions_rng.argtypes[6] == C.POINTER(N.McrAssumptions)
    assert lib.mcr_probe_assumptions_last_fanout_launches() == 0      # (no probe has run on this thread)
    assert lib.mcr_abi_version() == 8
