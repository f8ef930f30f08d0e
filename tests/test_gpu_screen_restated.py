"""The screening kernel's month as restated (csrc/mcr_screen.h, "the month as restated": one net need level per window state
chosen with scalar selects, the price level carried as a base-2 logarithm, the yearly contribution step behind a scalar branch,
a launch-constant rho = 0 form, no clamp on the two sold fractions, one running minimum of the balances folded into the class
where the class is read), on plans chosen for what those parts touch.  tests/test_screen_restated_cpu.py holds the same
restatement to the reference on the CPU; tests/test_gpu_screen_vs_oracle.py holds the kernel to the reference on random plans.

Plans (edits of scenarios/config.json; current_age 40, so retirement begins at row working_months and a window that opens at
age a begins at row 12 (a - 40)): every tax mask, mask 3 with equal and with unequal rates, each at rho = 0 and rho = 0.3 (the
ten screen_kernel instances); no income record, one and two, with windows that open before retirement, open and close inside
it, have zero length and never close, so that all four window states (neither, first, second, both) occur; contribution growth
on and off; working_months 0, 1, 12, 13 and 233 (even and odd month counts: a last row pair with one month); an all-safe plan
and the nearly-all-doubtful one (expenses 40 000).  Every other plan's monthly_expenses was set on the CPU with
tests/screen_model.py so that the fp64 model calls at least 64 of paths 0 .. 4095 SAFE and at least 64 DOUBTFUL.

Sizes: 300 and 4 096 paths, 4 096 paths across 2^32 and 4 096 paths from 5 10^9, all under MCR_K1_SCREEN=1.

Counts: `counters`, `wr_obs_counts` and `ruin_year_bins` of the screened route equal the classic route's (MCR_K1_SCREEN=0) and
the CPU oracle's exactly.

Classification (engine.screen_paths, the kernel alone), by the rule of tests/test_gpu_screen_vs_oracle.py: the class equals the
fp64 model's on every path whose `slack` is further than the plan's tolerance from 1; every kernel-SAFE path succeeds in the
oracle with no ruin year; on the paths SAFE in both, `min_ratio` and `final_total` are within the tolerance of the model's;
the lowest kernel `min_ratio` among SAFE keeps the margin.  The tolerance is max(2e-4, 8 x the deviation of the model's float32
run from its fp64 run), from the reference alone; at most 1 % of a plan's paths are excused by slack, here and on the random
plans of tests/count_fuzz.py.  The nearly-all-doubtful plan has fewer than 10 % SAFE paths and leaves the loop early (at
4 096 paths at least half its lanes stop holding more than the initial balance, where a path run to its end is ruined), the
all-safe plan has no doubtful path.

Observed on MI355X: LABNOTES R33."""

from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest

import count_fuzz as F
import screen_model
from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

pytestmark = pytest.mark.gpu

SEED, STREAM = 12345, 1
COUNT_KEYS = ("counters", "wr_obs_counts", "ruin_year_bins")
KEPT_MARGIN = 24.0 * (1.0 - 1e-5)       # cap x rcp(need) against cap >= 24 need: an fp32 rounding apart (tests/test_gpu_screen.py)
EXCUSED_MAX = 0.01


def _config(**over):
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        return dict(json.load(fh), **over)


def _stream(amount, start, years=None, tax=0.2):
    return {"name": f"s{amount}", "monthly_amount_today": amount, "start_at_age": start, "duration_years": years,
            "inflation_indexed": True, "tax_rate": tax}


PENSION = _config()["other_income_streams"][0]      # 4 000 a month from age 65 (row 300), indexed, no end
RHO = {"equity_inflation_correlation": 0.3}
UNEQUAL = {"inv2_realized_gains_tax_rate": 0.15}
MASK0 = {"inv1_use_realized_gains_tax_system": False, "inv2_use_realized_gains_tax_system": False}
MASK1 = {"inv2_use_realized_gains_tax_system": False}
MASK2 = {"inv1_use_realized_gains_tax_system": False}
NO_GROWTH = {"contribution_growth_rate_annual": 0.0}
INSIDE = [_stream(3000.0, 63.0, years=10, tax=0.275), _stream(2500.0, 70.5, years=12, tax=0.1)]     # rows 276..396 and 366..510: all four states
BEFORE = [_stream(2000.0, 50.0), _stream(2500.0, 70.5, years=12, tax=0.1)]                         # row 120 saturates at 233, never closes
ZERO = [_stream(3000.0, 62.0, years=0), PENSION]                                                   # a window of zero length, one that never closes

#         name                              config                                                                              working_months
PLANS = {
    "mask 3 equal rho 0 config.json":     (_config(),                                                                           233),
    "mask 3 equal rho 0.3 inside":        (_config(monthly_expenses=11000.0, other_income_streams=INSIDE, **RHO),                233),
    "mask 3 unequal rho 0 before":        (_config(monthly_expenses=11000.0, other_income_streams=BEFORE, **UNEQUAL),            233),
    "mask 3 unequal rho 0.3 wm 13":       (_config(monthly_expenses=1700.0, other_income_streams=ZERO, **UNEQUAL, **RHO),        13),
    "mask 0 rho 0 no record wm 12":       (_config(monthly_expenses=1400.0, other_income_streams=[], **MASK0, **NO_GROWTH),       12),
    "mask 0 rho 0.3 inside":              (_config(monthly_expenses=12500.0, other_income_streams=INSIDE, **MASK0, **RHO),       233),
    "mask 1 rho 0 wm 1":                  (_config(monthly_expenses=1300.0, **MASK1),                                            1),
    "mask 1 rho 0.3 no growth":           (_config(monthly_expenses=10000.0, **MASK1, **RHO, **NO_GROWTH),                        233),
    "mask 2 rho 0 wm 0":                  (_config(monthly_expenses=2000.0, other_income_streams=BEFORE, **MASK2),               0),
    "mask 2 rho 0.3 zero length":         (_config(monthly_expenses=11500.0, other_income_streams=ZERO, **MASK2, **RHO),         233),
    "all safe":                           (_config(initial_balance=1.0e9),                                                       233),
    "nearly all doubtful":                (_config(monthly_expenses=40000.0),                                                    233),
}
EACH_CLASS_MIN = 64                     # SAFE and DOUBTFUL paths of the fp64 model among paths 0 .. 4095, every plan but the last two
#         name                  first path      paths
SIZES = {
    "300":                      (0,             300),
    "4096":                     (0,             4096),
    "4096 across 2^32":         (2**32 - 2000,  4096),
    "4096 from 5e9":            (5 * 10**9,     4096),
}
N_MODEL = 4096


def _params(plan):
    cfgd, wm = PLANS[plan]
    return params_from_config(Config(**cfgd)), cfgd, wm


@functools.lru_cache(maxsize=None)
def _oracle(plan, begin, n):
    from oracle import oracle as O

    p, _, wm = _params(plan)
    return O.run_batch(p, SEED, STREAM, begin, n, wm, want_summary=True, want_trajectories=False)


@functools.lru_cache(maxsize=None)
def _reference(plan, begin):
    """count_fuzz.screen_reference for a plan of this file: the model in fp64 and float32 over N_MODEL paths from `begin`, their
    deviation on the paths SAFE in both, and the plan's tolerance."""
    p, cfgd, wm = _params(plan)
    fp64, fp32 = (screen_model.model(p, cfgd, wm, SEED, STREAM, begin, N_MODEL, dtype=t) for t in (np.float64, np.float32))
    both = fp64["safe"] & fp32["safe"]
    dev = 0.0
    for k in ("min_ratio", "final_total"):
        a, b = fp64[k][both], fp32[k][both].astype(np.float64)
        finite = np.isfinite(a)
        assert np.array_equal(finite, np.isfinite(b)), (plan, k)
        if finite.any():
            dev = max(dev, float(np.abs(b[finite] / a[finite] - 1.0).max()))
    return {"fp64": fp64, "dev": dev, "tol": max(F.SCREENED_TOL_FLOOR, F.SCREENED_TOL_FACTOR * dev)}


def _run(p, wm, begin, n, env):
    old = {k: os.environ.get(k) for k in F.SCREEN_KNOBS}
    for k in F.SCREEN_KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        assert E.screen(p, wm, n) == (env["MCR_K1_SCREEN"] == "1")
        r = E.run_batch_host(p, SEED, STREAM, begin, n, wm, want_summary=False, want_trajectories=False)
        return np.concatenate([np.asarray(r[k]).astype(np.int64) for k in COUNT_KEYS])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("plan", list(PLANS))
def test_counts_and_classes_of_the_restated_month(plan, size):
    begin, n = SIZES[size]
    p, cfgd, wm = _params(plan)
    ora = _oracle(plan, begin, n)
    want = np.concatenate([np.asarray(ora[k]).astype(np.int64) for k in COUNT_KEYS])
    classic = _run(p, wm, begin, n, {"MCR_K1_SCREEN": "0"})
    screened = _run(p, wm, begin, n, {"MCR_K1_SCREEN": "1"})
    assert int(classic[1]) == n
    assert np.array_equal(classic, want), (plan, "classic route vs oracle", np.nonzero(classic != want)[0][:8].tolist())
    assert np.array_equal(screened, classic), (plan, "screened route vs classic route", np.nonzero(screened != classic)[0][:8].tolist())

    ref = _reference(plan, begin)
    m, tol = {k: v[:n] for k, v in ref["fp64"].items()}, ref["tol"]
    assert tol <= F.SCREENED_TOL_MAX, (plan, tol)
    k = E.screen_paths(p, SEED, STREAM, begin, n, wm)
    assert set(np.unique(k["cls"]).tolist()) <= {0, 1}
    safe = k["cls"] == 0
    decided = np.abs(m["slack"] - 1.0) > tol
    excused = int((~decided).sum())
    both = safe & m["safe"]
    no_need = np.isinf(m["min_ratio"][both])
    rel = lambda got, want: float(np.abs(got.astype(np.float64) / want - 1.0).max()) if got.size else 0.0      # noqa: E731
    d_total = rel(k["final_total"][both], m["final_total"][both])
    d_ratio = rel(k["min_ratio"][both][~no_need], m["min_ratio"][both][~no_need])
    low = float(k["min_ratio"][safe].min()) if safe.any() else float("inf")
    print(f"  {plan}, {size}: SAFE model {int(m['safe'].sum())} kernel {int(safe.sum())} of {n}, excused by slack {excused} "
          f"(classes differ on {int((~decided & (safe != m['safe'])).sum())}), tol {tol:.2e} (dev {ref['dev']:.2e}), "
          f"max dev min_ratio {d_ratio:.2e} final_total {d_total:.2e}, lowest min_ratio among SAFE {low:.3f}")
    wrong = decided & (safe != m["safe"])
    assert not wrong.any(), ("class", np.nonzero(wrong)[0][:8].tolist(), m["slack"][wrong][:8].tolist())
    assert excused <= EXCUSED_MAX * n, (excused, n)
    assert np.all(ora["success"][safe] == 1) and np.all(np.isnan(ora["years_to_ruin"][safe])), np.nonzero(safe & (ora["success"] == 0))[0][:8].tolist()
    assert np.array_equal(np.isinf(k["min_ratio"][both]), no_need)
    assert d_ratio <= tol, ("min_ratio", d_ratio, tol)
    assert d_total <= tol, ("final_total", d_total, tol)
    assert low >= KEPT_MARGIN, low
    if plan == "all safe":
        assert safe.all() and int(screened[0]) == n
    elif plan == "nearly all doubtful":
        assert 10 * int(safe.sum()) < n
        if n == 4096:
            # 40 000 a month ruins a path that runs to its end (total zero, negative or NaN); a lane whose wave left the loop
            # at the first vote after its last lane turned doubtful still holds the savings of its accumulation years
            ft = k["final_total"]
            stopped = np.isfinite(ft) & (ft > cfgd["initial_balance"])
            print(f"  {plan}: {int(stopped.sum())} of {n} lanes stopped with more than the initial balance (median total {float(np.median(ft[stopped])) if stopped.any() else 0.0:.3e})")
            assert int(stopped.sum()) >= n // 2, int(stopped.sum())
    elif size == "4096":
        assert EACH_CLASS_MIN <= int(m["safe"].sum()) <= n - EACH_CLASS_MIN, int(m["safe"].sum())


@pytest.mark.parametrize("base", F.SCREENED_BASES)
def test_the_random_plans_stay_within_the_excused_cap(oracle, base):
    """The paths of tests/count_fuzz.py's screened plans that the classification comparison of
    tests/test_gpu_screen_vs_oracle.py excuses by slack: at most 1 % of a plan's paths, at both levels."""
    for s in F.screened_scenarios(oracle, base):
        for level in F.SCREENED_LEVELS:
            ref = F.screen_reference(s, level)
            excused = int((np.abs(ref["fp64"]["slack"] - 1.0) <= ref["tol"]).sum())
            assert excused <= EXCUSED_MAX * s.n, (excused, s.context(level))
