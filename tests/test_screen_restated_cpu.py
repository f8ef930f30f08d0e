"""The screening kernel's month as restated (tests/screen_restated.py: one net need level per window state, the price level
carried as a base-2 logarithm, no clamp on the sold fractions, one running minimum of the balances, Box-Muller angles a
2^-23 revolution short) against the reference, tests/screen_model.py in fp64, on the 40 screened plans of tests/count_fuzz.py at
both expense levels — NumPy and the CPU oracle only, no device.  It decides on the CPU whether the restatement (the logarithmic
price level above all: 833 float32 additions) fits the plans' tolerances, before any kernel runs.

Per plan and level:
  * every path the restatement calls SAFE succeeds in the oracle with no ruin year;
  * on the paths SAFE in both the restatement and the fp64 model, `min_ratio` and `final_total` deviate by at most the plan's
    `tol` (count_fuzz.screen_reference: max(2e-4, 8 x the deviation of the REFERENCE's float32 run), from screen_model alone);
    `min_ratio` is inf in both or in neither;
  * the classes differ from the fp64 model's only where the model's `slack` is within `tol` of 1.

Observed (seed 20261018): LABNOTES R33, "restatement on the CPU"."""

from __future__ import annotations

import numpy as np
import pytest

import count_fuzz as F
import screen_restated


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in F.SCREEN_KNOBS:
        monkeypatch.delenv(k, raising=False)


def _dev(got, want):
    finite = np.isfinite(want)
    assert np.array_equal(finite, np.isfinite(got))
    return float(np.abs(got[finite].astype(np.float64) / want[finite] - 1.0).max()) if finite.any() else 0.0


@pytest.mark.parametrize("base", F.SCREENED_BASES)
def test_the_restated_month_keeps_the_reference_within_each_plans_tolerance(oracle, base):
    plans = F.screened_scenarios(oracle, base)
    F.oracle_runs(oracle, [((F.at_level(s, level),), {}) for s in plans for level in F.SCREENED_LEVELS])
    worst = worst_ref = 0.0
    for level in F.SCREENED_LEVELS:
        for s in plans:
            at = F.at_level(s, level)
            ref = F.screen_reference(s, level)
            m, tol = ref["fp64"], ref["tol"]
            ora = F.oracle_run(oracle, at)
            r = screen_restated.model(at.params(), at.cfgd, at.wm, at.seed, at.stream, at.begin, at.n, angle=True)
            safe = r["safe"]
            assert np.all(ora["success"][safe] == 1) and np.all(np.isnan(ora["years_to_ruin"][safe])), at.context(level)
            decided = np.abs(m["slack"] - 1.0) > tol
            assert not np.any(decided & (safe != m["safe"])), at.context(level)
            both = safe & m["safe"]
            d = max(_dev(r["min_ratio"][both], m["min_ratio"][both]), _dev(r["final_total"][both], m["final_total"][both]))
            print(f"  {at.cfgd['scenario']} {level}: SAFE model {int(m['safe'].sum())} restated {int(safe.sum())} of {at.n}, "
                  f"deviation {d:.2e} (reference float32 {ref['dev']:.2e}, tol {tol:.2e})")
            assert d <= tol, (d, tol, at.context(level))
            if F.screened_edge(s) is not None:
                assert not safe.any(), at.context(level)
            worst, worst_ref = max(worst, d), max(worst_ref, ref["dev"])
    print(f"{base}: largest deviation of the restated month {worst:.2e}, of the reference's float32 run {worst_ref:.2e}")
