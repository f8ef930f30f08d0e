"""The screening kernel after its second restatement (csrc/mcr_screen.h, "the month as restated": four rows to a loop
iteration with the Philox pair carry local to it, the Box-Muller radius constant folded into the growth slopes, the net levels
clamped where they are derived, one compare against max(24 need, peak / 64), the rebalanced balances in closed form), on the
smallest plans at which the new loop and the folded constants can go wrong.  tests/test_screen_month2_cpu.py holds the same
arithmetic to the reference on the CPU.

Plans (edits of scenarios/config.json; current_age 40, so retirement begins at row working_months and a window that opens at
age a begins at row 12 (a - 40)): working_months 232, 233, 234 and 235 — total_months = working_months + 12 x 50, so every residue
of total_months % 4 occurs (the loop's three early exits and the full group) and the retirement boundary falls at every position
of a four-row group; 228, a multiple of 12, where the last yearly contribution step meets the boundary, beside the four that are
not; income windows that open and close at rows 279, 399 (position 3 of a group) and 369, 513 (position 1), at rows 276, 396
and 366, 510 (positions 0 and 2), one of zero length and one that never closes; rho 0 and 0.3; tax masks 0 to 3, mask 3 with
equal and with unequal rates.  Each plan's monthly_expenses was chosen on the CPU (count_fuzz._calibrate at a failing share of
0.05, then tests/screen_model.py in fp64) so that the model calls at least 64 of paths 0 .. 4095 SAFE and at least 64 DOUBTFUL;
the test asserts it.

Sizes: 300 paths (tail lanes), 4 096, 4 096 across 2^32 (the non-uniform Philox form) and 4 096 from 5 10^9.

Per case: `counters`, `wr_obs_counts` and `ruin_year_bins` under MCR_K1_SCREEN=1 equal those under MCR_K1_SCREEN=0 and the CPU
oracle's, exactly; through engine.screen_paths the kernel's class, `min_ratio` and `final_total` are held to the fp64 model by
the rule of tests/test_gpu_screen_vs_oracle.py: the tolerance is max(2e-4, 8 x the deviation of the model's float32 run from its
fp64 run), a class may differ only where the model's `slack` is within it of 1, and at most 1 % of a case's paths are so excused.

Observed on MI355X: LABNOTES R34."""

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
EACH_CLASS_MIN = 64                     # SAFE and DOUBTFUL paths of the fp64 model among paths 0 .. 4095, every plan
N_MODEL = 4096


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
INSIDE = [_stream(3000.0, 63.0, years=10, tax=0.275), _stream(2500.0, 70.5, years=12, tax=0.1)]      # rows 276..396 and 366..510
ODD = [_stream(3000.0, 63.25, years=10, tax=0.275), _stream(2500.0, 70.75, years=12, tax=0.1)]       # rows 279..399 and 369..513
ZERO = [_stream(3000.0, 62.0, years=0), PENSION]                                                    # a window of zero length, one that never closes

#         name                              config                                                                              working_months
PLANS = {
    "mask 3 equal rho 0 wm 232":          (_config(monthly_expenses=10330.0),                                                   232),
    "mask 3 equal rho 0.3 odd wm 233":    (_config(monthly_expenses=9780.0, other_income_streams=ODD, **RHO),                   233),
    "mask 3 unequal rho 0 zero wm 234":   (_config(monthly_expenses=10230.0, other_income_streams=ZERO, **UNEQUAL),             234),
    "mask 3 unequal rho 0.3 inside 235":  (_config(monthly_expenses=9700.0, other_income_streams=INSIDE, **UNEQUAL, **RHO),     235),
    "mask 0 rho 0 odd wm 228":            (_config(monthly_expenses=10510.0, other_income_streams=ODD, **MASK0),                228),
    "mask 0 rho 0.3 wm 234":              (_config(monthly_expenses=11610.0, **MASK0, **RHO),                                   234),
    "mask 1 rho 0.3 inside wm 232":       (_config(monthly_expenses=10140.0, other_income_streams=INSIDE, **MASK1, **RHO),      232),
    "mask 2 rho 0 odd wm 235":            (_config(monthly_expenses=10420.0, other_income_streams=ODD, **MASK2),                235),
}
#         name                  first path      paths
SIZES = {
    "300":                      (0,             300),
    "4096":                     (0,             4096),
    "4096 across 2^32":         (2**32 - 2000,  4096),
    "4096 from 5e9":            (5 * 10**9,     4096),
}


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


def test_the_plans_cover_every_group_position():
    residues = {(wm + 12 * cfgd["retirement_years"]) % 4 for cfgd, wm in PLANS.values()}
    assert residues == {0, 1, 2, 3}
    assert {wm % 4 for _, wm in PLANS.values()} == {0, 1, 2, 3}
    assert any(wm % 12 == 0 for _, wm in PLANS.values()) and any(wm % 12 != 0 for _, wm in PLANS.values())


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("plan", list(PLANS))
def test_counts_and_classes_of_the_second_restatement(plan, size):
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
    if size == "4096":
        assert EACH_CLASS_MIN <= int(m["safe"].sum()) <= n - EACH_CLASS_MIN, int(m["safe"].sum())
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
