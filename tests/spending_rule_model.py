"""The spending rule of include/mcr.h held to the UNMODIFIED CPU oracle — a helper of the spending-rule tests, not a test.

A year-by-year multiplier history ``m_0 .. m_{ry-1}`` is a deterministic expense schedule, and the oracle can run such a
schedule as it stands: base expenses ``E max(m)`` minus inflation-indexed, tax-free income streams of ``E (max(m) - m_y)`` over
the years where ``m_y`` is lower (`scheduled_params`).  So

* `verify` judges a path the GPU ran under a rule: one oracle run of the path under the GPU's own multiplier row must give the
  GPU's outcome, and every year's multiplier must be what the rule decides from the oracle's own yearly sample;
* `model` builds a path's multipliers on the CPU alone, year by year: run the oracle, decide year y, extend the schedule.

The rule (include/mcr.h, ``mcr_spending_rule``): with ``r0 = start_balance / inflation_at_retirement`` and ``R`` = the real
balance at the start of retirement year ``y >= 1`` (``real_trajectory`` sample of the end of year ``y - 1``), a path that begins
the year alive cuts when ``m r0 > upper R``, raises when ``m r0 < lower R``.  The kernel evaluates the same comparison on the
nominal balance and the price level, ``(m r0) P`` against ``upper B``; the two differ by roundings, and a decision that a
change of the balance by the differential test's bound would flip is UNDECIDABLE: either outcome is accepted.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from monte_carlo_retirement_amd._native import McrParams
from oracle import oracle as O
from test_gpu_differential import ABS, REL   # the bound of the differential test: imported, not restated

EPS = 1e-6          # MCR_SMALL_EPSILON
CUT, KEEP, RAISE = -1, 0, 1


def rule_values(rule) -> Tuple[float, float, float, float, float, float]:
    """(upper, lower, cut, raise, floor, ceiling) of a `SpendingRule` or a plain 6-sequence."""
    if hasattr(rule, "upper"):
        return (rule.upper, rule.lower, rule.cut, rule.raise_, rule.floor, rule.ceiling)
    return tuple(float(x) for x in rule)   # type: ignore[return-value]


def decide(rule, m: float, r0: float, real_balance: float) -> int:
    upper, lower = rule_values(rule)[:2]
    lhs = m * r0
    if lhs > upper * real_balance:
        return CUT
    if lhs < lower * real_balance:
        return RAISE
    return KEEP


def apply(rule, m: float, decision: int) -> float:
    """The multiplier after a decision: the header's two expressions, the same fp64 operations."""
    _, _, cut, raise_, floor, ceiling = rule_values(rule)
    if decision == CUT:
        return max(floor, m * (1.0 - cut))
    if decision == RAISE:
        return min(ceiling, m * (1.0 + raise_))
    return m


def copy_params(p: McrParams) -> McrParams:
    q = McrParams()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(McrParams))
    q._extra_keepalive = p._extra_keepalive
    return q


def stream_records(p: McrParams) -> List[tuple]:
    out = []
    for i in range(p.n_streams):
        s = p.stream(i)
        out.append((s.monthly_amount_today, s.start_at_age, s.tax_rate, None if s.duration_years < 0 else s.duration_years,
                    bool(s.inflation_indexed)))
    return out


def scheduled_params(params: McrParams, wm: int, multipliers: Sequence[float]) -> McrParams:
    """`params` with the expense schedule ``monthly_expenses * multipliers[y]`` in retirement year y, in the oracle's own
    terms: expenses ``E max(m)`` and one indexed, untaxed stream of ``E (max(m) - m_y)`` per run of equal neighbouring years
    with ``m_y < max(m)``, starting at retirement age + y.  Every stream must start at month ``12 y`` of retirement."""
    m = [float(x) for x in multipliers]
    assert len(m) == params.retirement_years and all(np.isfinite(m))
    q = copy_params(params)
    top = max(m)
    E = params.monthly_expenses
    q.monthly_expenses = E * top
    records = stream_records(params)
    retirement_age = params.current_age + wm / 12.0
    y = 0
    while y < len(m):
        z = y
        while z + 1 < len(m) and m[z + 1] == m[y]:
            z += 1
        if m[y] < top:
            start = retirement_age + y
            assert O.stream_start_month_index(params.current_age, wm, start) == 12 * y, (wm, y, start)
            records.append((E * (top - m[y]), start, 0.0, z - y + 1, True))
        y = z + 1
    q.set_streams(records)
    return q


def run_path(params: McrParams, wm: int, seed: int, stream_id: int, path: int, multipliers: Sequence[float]) -> Dict[str, np.ndarray]:
    """One oracle run of one path under a multiplier schedule; arrays as `oracle.run_batch` returns them, one column."""
    return O.run_batch(scheduled_params(params, wm, multipliers), seed, stream_id, path, 1, wm)


def begins_year(years_to_ruin: float, y: int) -> bool:
    """Whether a path with that YearsToRuin begins retirement year y alive (a failure in year y' gives a value in (y', y' + 1],
    a pre-retirement failure 0.0, a failure at the terminal settlement retirement_years)."""
    return bool(np.isnan(years_to_ruin) or years_to_ruin > y)


def _money_scale(run) -> float:
    return float(max(1.0, np.abs(run["trajectory"][:, 0]).max()))


def model(params: McrParams, wm: int, rule, seed: int, stream_id: int, path: int):
    """The path's multipliers under `rule` from the oracle alone, year by year.  Returns ``(row, run)``: ``row[y]`` = m of year y,
    NaN for a year the path does not begin; ``run`` = the oracle's run of the final schedule."""
    ry = int(params.retirement_years)
    m = [1.0] * ry
    run = run_path(params, wm, seed, stream_id, path, m)
    if rule_values(rule)[2] != 0.0 or rule_values(rule)[3] != 0.0:
        T = run["trajectory"].shape[0]
        for y in range(1, ry):
            if not begins_year(float(run["years_to_ruin"][0]), y):
                break
            b0, p0 = float(run["start_balance"][0]), float(run["inflation_at_retirement"][0])
            if b0 <= EPS:
                break
            new = apply(rule, m[y - 1], decide(rule, m[y - 1], b0 / p0, float(run["real_trajectory"][T - ry + y - 1, 0])))
            if new != m[y]:
                m[y:] = [new] * (ry - y)
                run = run_path(params, wm, seed, stream_id, path, m)
            # (the schedule beyond year y does not reach back: the years before y ran as they will run)
    ytr = float(run["years_to_ruin"][0])
    row = np.array([m[y] if begins_year(ytr, y) else np.nan for y in range(ry)], dtype=np.float64)
    return row, run


def verify(params: McrParams, wm: int, rule, seed: int, stream_id: int, path: int, multipliers_row, outcome) -> bool:
    """Judge one path the engine ran under `rule`.  ``multipliers_row``: its ``[ry]`` multipliers (NaN where it does not begin
    the year); ``outcome``: ``{"success", "years_to_ruin", "final_balance"}`` of its summary.  One oracle run of the path under
    that schedule: the success flag and YearsToRuin must agree exactly, the final balance within ``ABS + REL max(|c|, the path's
    money scale)``, and every year's multiplier must be the rule's decision on the oracle's own sample of the year before.
    Raises AssertionError; returns whether any year was undecidable."""
    ry = int(params.retirement_years)
    row = np.asarray(multipliers_row, dtype=np.float64)
    assert row.shape == (ry,), row.shape
    ctx = f"path {path} wm {wm}"
    # the schedule the oracle runs: the row, years the path does not begin filled with the last multiplier it had
    sched, last = [], 1.0
    for y in range(ry):
        if not np.isnan(row[y]):
            last = float(row[y])
        sched.append(last)
    run = run_path(params, wm, seed, stream_id, path, sched)
    c_ok, c_ytr, c_fin = bool(run["success"][0]), float(run["years_to_ruin"][0]), float(run["final_balance"][0])
    assert bool(outcome["success"]) == c_ok, (ctx, "success", bool(outcome["success"]), c_ok)
    g_ytr = float(outcome["years_to_ruin"])
    assert (np.isnan(g_ytr) and np.isnan(c_ytr)) or g_ytr == c_ytr, (ctx, "years_to_ruin", g_ytr, c_ytr)
    scale = _money_scale(run)
    assert abs(float(outcome["final_balance"]) - c_fin) <= ABS + REL * max(abs(c_fin), scale), (ctx, "final_balance", float(outcome["final_balance"]), c_fin)
    T = run["trajectory"].shape[0]
    b0, p0 = float(run["start_balance"][0]), float(run["inflation_at_retirement"][0])
    inert = b0 <= EPS
    undecidable = False
    for y in range(ry):
        begun = begins_year(c_ytr, y)
        assert np.isnan(row[y]) == (not begun), (ctx, "year", y, "begun", begun, float(row[y]))
        if not begun:
            continue
        if y == 0 or inert:
            want = {1.0}
        else:
            prev = float(row[y - 1])
            R = float(run["real_trajectory"][T - ry + y - 1, 0])
            tol = ABS + REL * max(abs(R), scale)
            decisions = {decide(rule, prev, b0 / p0, R), decide(rule, prev, b0 / p0, R - tol), decide(rule, prev, b0 / p0, R + tol)}
            undecidable = undecidable or len(decisions) > 1
            want = {apply(rule, prev, d) for d in decisions}
        assert float(row[y]) in want, (ctx, "year", y, "multiplier", float(row[y]), "rule gives", sorted(want))
    return undecidable


def year_counts_of(rows: np.ndarray, rule) -> np.ndarray:
    """``[ry, 4]`` {alive, cut, at the floor, raised} recomputed from multiplier rows ``[ry, n]``."""
    floor = rule_values(rule)[4]
    begun = ~np.isnan(rows)
    with np.errstate(invalid="ignore"):
        return np.stack([begun.sum(axis=1), (begun & (rows < 1.0)).sum(axis=1),
                         (begun & (rows <= floor)).sum(axis=1) if floor < 1.0 else np.zeros(rows.shape[0], dtype=np.int64),
                         (begun & (rows > 1.0)).sum(axis=1)], axis=1).astype(np.int64)


# ---- the plans and rules of the spending-rule tests -----------------------------------------------------------------------
RULES = {"neutral": (1.0, 1.0, 0.0, 0.0, 1.0, 1.0), "cut_only": (1.0, 0.0, 0.10, 0.0, 0.6, 1.0),
         "symmetric": (1.2, 0.8, 0.10, 0.10, 0.5, 1.5)}


#: monthly_expenses per (plan, working_months), by rule.  Calibrated on the CPU alone (the oracle, and `model` for the firing
#: rules) on paths 0 .. 599 of seed 20260, stream 1: at these levels between 10 % and 90 % of the paths fail under their rule, and
#: under the firing rules more than 5 % of the begun path-years are cut, some stand at the floor, some are raised under the
#: symmetric rule, and `verify` finds no undecidable year in the model's rows.
LEVELS = {("realized", 0): {"neutral": 1113.0, "cut_only": 1590.0, "symmetric": 1590.0},
          ("realized", 7): {"neutral": 1295.0, "cut_only": 1850.0, "symmetric": 1850.0},
          ("realized", 120): {"neutral": 4690.0, "cut_only": 6700.0, "symmetric": 6700.0},
          ("annual", 0): {"neutral": 1015.0, "cut_only": 1450.0, "symmetric": 1450.0},
          ("annual", 7): {"neutral": 1176.0, "cut_only": 1680.0, "symmetric": 1680.0},
          ("annual", 120): {"neutral": 4025.0, "cut_only": 5750.0, "symmetric": 5750.0},
          ("streams", 0): {"neutral": 2310.0, "cut_only": 3300.0, "symmetric": 3650.0},
          ("streams", 7): {"neutral": 2520.0, "cut_only": 3600.0, "symmetric": 3950.0},
          ("streams", 120): {"neutral": 6020.0, "cut_only": 8600.0, "symmetric": 8600.0}}
SEED, STREAM = 20260, 1


def plan_config(name: str, repo: str, wm: int = 0) -> dict:
    """config.json with 30 retirement years and: "realized" = realized-gains tax on both assets (its own 10 %); "annual" =
    an annual gains tax on both assets instead; "streams" = two income streams, one frozen-nominal, that start in retirement
    year 5 when retiring after `wm` months."""
    import json
    import os

    with open(os.path.join(repo, "scenarios", "config.json")) as fh:
        cfg = json.load(fh)
    # (config.json's own volatilities, 2 %, leave every path of a plan on one side of a guardrail: the markets here move enough
    #  for one plan to hold paths that are cut, paths that are raised and paths that are left alone)
    cfg.update(retirement_years=30, seed=20260, num_processes=1, inv1_returns_volatility=0.16,
               inv2_premium_over_inflation_volatility=0.06)
    year5 = cfg["current_age"] + wm / 12.0 + 5.0
    if name == "realized":
        cfg["other_income_streams"] = []
    elif name == "annual":
        cfg.update(inv1_use_realized_gains_tax_system=False, inv1_annual_tax_on_gains_rate=0.15,
                   inv2_use_realized_gains_tax_system=False, inv2_annual_tax_on_gains_rate=0.15, other_income_streams=[])
    elif name == "streams":
        cfg["other_income_streams"] = [
            {"name": "annuity", "monthly_amount_today": 1500.0, "start_at_age": year5, "duration_years": None,
             "inflation_indexed": True, "tax_rate": 0.2},
            {"name": "lease", "monthly_amount_today": 1200.0, "start_at_age": year5, "duration_years": 12,
             "inflation_indexed": False, "tax_rate": 0.1}]
    else:
        raise ValueError(name)
    return cfg
