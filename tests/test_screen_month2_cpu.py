"""The screening kernel's month after its second restatement (tests/screen_month2.py: the Box-Muller radius constant folded
into the growth slopes, the net levels clamped where they are derived, one compare against max(24 need, peak / 64), the
rebalanced balances in closed form) against the reference, tests/screen_model.py in fp64, on the 40 screened plans of
tests/count_fuzz.py at both expense levels — NumPy and the CPU oracle only, no device.

Per plan and level, as tests/test_screen_restated_cpu.py holds the first restatement:
  * every path the restatement calls SAFE succeeds in the oracle with no ruin year;
  * on the paths SAFE in both the restatement and the fp64 model, `min_ratio` and `final_total` deviate by at most the plan's
    `tol` (count_fuzz.screen_reference: max(2e-4, 8 x the deviation of the REFERENCE's float32 run), from screen_model alone);
  * the classes differ from the fp64 model's only where the model's `slack` is within `tol` of 1;
and, exactly: the single compare gives the two compares' answer on every path in every month.

The largest deviation per tax base is printed next to the first restatement's (R33_DEVIATION, LABNOTES R33).
Observed (seed 20261018): LABNOTES R34, "restatement on the CPU"."""

from __future__ import annotations

import numpy as np
import pytest

import count_fuzz as F
import screen_month2

R33_DEVIATION = {"equal_rates": 5.1e-5, "unequal_rates": 2.3e-5, "mask1": 8.0e-5, "mask2": 4.8e-5, "mask0": 2.5e-4}


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in F.SCREEN_KNOBS:
        monkeypatch.delenv(k, raising=False)


def _dev(got, want):
    finite = np.isfinite(want)
    assert np.array_equal(finite, np.isfinite(got))
    return float(np.abs(got[finite].astype(np.float64) / want[finite] - 1.0).max()) if finite.any() else 0.0


@pytest.mark.parametrize("base", F.SCREENED_BASES)
def test_the_second_restatement_keeps_the_reference_within_each_plans_tolerance(oracle, base):
    plans = F.screened_scenarios(oracle, base)
    F.oracle_runs(oracle, [((F.at_level(s, level),), {}) for s in plans for level in F.SCREENED_LEVELS])
    worst = worst_ref = 0.0
    for level in F.SCREENED_LEVELS:
        for s in plans:
            at = F.at_level(s, level)
            ref = F.screen_reference(s, level)
            m, tol = ref["fp64"], ref["tol"]
            ora = F.oracle_run(oracle, at)
            r = screen_month2.model(at.params(), at.cfgd, at.wm, at.seed, at.stream, at.begin, at.n)
            safe = r["safe"]
            assert r["same_class"].all(), ("one compare against two", np.nonzero(~r["same_class"])[0][:8].tolist(), at.context(level))
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
    print(f"{base}: largest deviation of the second restatement {worst:.2e} (first restatement, R33: {R33_DEVIATION[base]:.1e}), "
          f"of the reference's float32 run {worst_ref:.2e}")
