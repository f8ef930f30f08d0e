"""The allocation options of tests/allocation_fuzz.py are worth running: the oracle alone, no device.

tests/test_gpu_allocation_vs_oracle.py compares the outcome and joint probes of the allocation family with the oracle's per-path
columns of these options.  That comparison is vacuous where an option moves no path, and its final-balance rows are thin where
an option leaves a plan all-or-nothing.  Measured with the suite's seed (68 plans):

    option    plans with a path whose outcome differs from the plan's own     plans with 5-95 % of the paths failing
    mirror    64                                                              40
    toward    66                                                              47
    zero      53                                                              33
    one       54                                                              47

No option run reaches the 2^33 money scale.  The floors below are conditions set under those figures, so that another seed or
another draw fails loudly here and not silently on the device."""

from __future__ import annotations

import time

import numpy as np

import allocation_fuzz as AF
import count_fuzz as F

#: option -> (plans with a discordant path at least, plans with mixed outcomes at least)
FLOORS = {"mirror": (55, 30), "toward": (55, 35), "zero": (45, 25), "one": (45, 35)}


def test_the_options_move_paths_and_leave_mixed_outcomes(oracle):
    t0 = time.time()
    discordant = {k: 0 for k in FLOORS}
    mixed = {k: 0 for k in FLOORS}
    over_scale, plans, runs_made = [], 0, 0
    for cls in F.CLASSES:
        for scn, runs in AF.class_runs(oracle, cls):
            plans += 1
            own = runs[0]
            assert own is F.oracle_run(oracle, scn, trajectories=True)          # the plan's own run, shared with every other test
            xs = AF.splits(scn)
            assert len(xs) == len(AF.NAMES) == len(runs) and all(0.0 <= x <= 1.0 for x in xs), (xs, scn.context())
            for name, run in zip(AF.NAMES, runs):
                runs_made += 1
                assert int(run["counters"][1]) == scn.n
                if F.money_scale(run) >= F.SCALE_LIMIT:
                    over_scale.append((name, scn.cls, scn.index))
                if name == "own":
                    continue
                discordant[name] += bool(np.any(run["success"] != own["success"]))
                mixed[name] += F.MIXED[0] <= F.failure_share(run) <= F.MIXED[1]
    print(f"allocation_fuzz, count_fuzz seed {F.seed()}: {plans} plans, {runs_made} option runs with trajectories in {time.time() - t0:.1f} s "
          f"(0.0 where another test made them), {len(over_scale)} over the 2^33 money scale")
    for key in FLOORS:
        print(f"  {key}: plans with a path whose outcome differs from the plan's own {discordant[key]}, plans with mixed outcomes {mixed[key]}")
    assert plans == 68
    assert not over_scale, over_scale
    for key, (least_discordant, least_mixed) in FLOORS.items():
        assert discordant[key] >= least_discordant, (key, discordant[key])
        assert mixed[key] >= least_mixed, (key, mixed[key])
