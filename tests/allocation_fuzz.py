"""Allocation options for the stratified random plans of tests/count_fuzz.py, with the CPU oracle's answer to each.

An allocation option is a `Config` override the unmodified ORACLE can run, so its per-path columns are the reference of
tests/test_gpu_allocation_vs_oracle.py, and tests/test_allocation_fuzz_cpu.py shows from the oracle alone that the options are
worth running: they move paths, and they leave most plans with both outcomes.

Options of a plan whose own split is a (`allocation_inv1_pct`; the three amounts stay the plan's own):
    own:     a
    mirror:  1 - a
    toward:  a + 0.35 if a < 0.5, else a - 0.35
    zero:    0.0   (everything in the second asset: the first one's balance is dust from month 0)
    one:     1.0"""

from __future__ import annotations

import count_fuzz as F
from option_fuzz import SCENARIO_FIELDS, oracle_flags, oracle_rows  # noqa: F401  (the same rows and flags, re-exported)

NAMES = ("own", "mirror", "toward", "zero", "one")


def splits(scn):
    a = float(scn.cfgd["allocation_inv1_pct"])
    return [a, 1.0 - a, a + 0.35 if a < 0.5 else a - 0.35, 0.0, 1.0]


def overrides(scn):
    """The `Config` fields each option replaces: one dict per option, {} for the plan's own."""
    return [{}] + [{"allocation_inv1_pct": x} for x in splits(scn)[1:]]


def records(scn):
    """The options as the probe takes them."""
    own = tuple(float(scn.cfgd[f]) for f in SCENARIO_FIELDS)
    return [own + (float(x),) for x in splits(scn)]


def class_runs(O, cls):
    """[(plan, [the oracle's trajectory run of each option])] of class `cls`: on host threads, cached by count_fuzz."""
    plans = F.scenarios(O, cls)
    jobs = [((scn,), dict(trajectories=True, **o)) for scn in plans for o in overrides(scn)]
    runs = F.oracle_runs(O, jobs)
    n = len(NAMES)
    return [(scn, runs[n * k: n * k + n]) for k, scn in enumerate(plans)]
