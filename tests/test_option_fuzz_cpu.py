"""The scenario and assumption options of tests/option_fuzz.py are worth running: the oracle alone, no device.

tests/test_gpu_probe_options_vs_oracle.py compares the outcome and joint probes of both families with the oracle's per-path
columns of these options.  That comparison is vacuous where an option moves no path, and its final-balance rows are thin where
an option leaves a plan all-or-nothing.  Measured with the suite's seed (68 plans):

    option          plans with a path whose outcome differs from the plan's own     plans with 5-95 % of the paths failing
    A               67                                                              38
    B               67                                                              35
    market record   60                                                              58

No option run reaches the 2^33 money scale.  The floors below are conditions set under those figures, so that another seed or
another draw fails loudly here and not silently on the device."""

from __future__ import annotations

import time

import numpy as np

import count_fuzz as F
import option_fuzz as OF

#: option -> (plans with a discordant path at least, plans with mixed outcomes at least)
FLOORS = {("scenarios", "A"): (60, 30), ("scenarios", "B"): (60, 30), ("assumptions", "market"): (50, 50)}


def test_the_options_move_paths_and_leave_mixed_outcomes(oracle):
    t0 = time.time()
    discordant = {k: 0 for k in FLOORS}
    mixed = {k: 0 for k in FLOORS}
    over_scale, plans, runs_made, months = [], 0, 0, set()
    for family in OF.FAMILIES:
        for cls in F.CLASSES:
            for scn, runs in OF.class_runs(oracle, cls, family):
                plans += family == "scenarios"
                own = runs[0]
                assert own is F.oracle_run(oracle, scn, trajectories=True)          # the plan's own run, shared with every other test
                for name, run in zip(OF.NAMES[family], runs):
                    runs_made += 1
                    assert int(run["counters"][1]) == scn.n
                    if F.money_scale(run) >= F.SCALE_LIMIT:
                        over_scale.append((family, name, scn.cls, scn.index))
                    bad = ~np.isnan(run["years_to_ruin"])
                    months.update(np.rint(12.0 * run["years_to_ruin"][bad]).astype(np.int64).tolist())
                    if name == "own":
                        continue
                    discordant[family, name] += bool(np.any(run["success"] != own["success"]))
                    mixed[family, name] += F.MIXED[0] <= F.failure_share(run) <= F.MIXED[1]
    print(f"option_fuzz, count_fuzz seed {F.seed()}: {plans} plans, {runs_made} option runs with trajectories in {time.time() - t0:.1f} s "
          f"(0.0 where another test made them), {len(over_scale)} over the 2^33 money scale, {len(months)} distinct ruin months")
    for key in FLOORS:
        print(f"  {key[0]} {key[1]}: plans with a path whose outcome differs from the plan's own {discordant[key]}, plans with mixed outcomes {mixed[key]}")
    assert plans == 68
    assert not over_scale, over_scale
    for key, (least_discordant, least_mixed) in FLOORS.items():
        assert discordant[key] >= least_discordant, (key, discordant[key])
        assert mixed[key] >= least_mixed, (key, mixed[key])
    assert len(months) >= 100 and 0 in months, len(months)
