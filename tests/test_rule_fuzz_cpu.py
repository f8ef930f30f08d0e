"""The cases tests/rule_fuzz.py generates are worth running before a GPU sees them: mixed outcomes under their rules, cuts, floors
and raises, a rule that can only keep m = 1, paths that fail before retirement, path ranges across the 32-bit word of the Philox
counter, and a CPU model (`spending_rule_model.model`) whose own rows pass its own judge (`verify`) with no undecidable year to
speak of.  The generator, the CPU oracle and the model only: no device needed.

These are conditions on the family, decided before any kernel ran; the figures of the suite's seed are printed (`-s`)."""

from __future__ import annotations

import time

import numpy as np

import count_fuzz as F
import rule_fuzz as RF


def test_the_cases_meet_their_conditions(oracle):
    t0 = time.time()
    cases = RF.all_cases(oracle)
    t1 = time.time()
    answers = {c.id: RF.answer(oracle, c) for c in cases}
    t2 = time.time()
    assert len(cases) == len(RF.CLASSES) * RF.PER_CLASS == 36 and [c.k for c in cases] == list(range(36))
    undecidable = {}
    for c in cases:
        a = answers[c.id]
        flags = RF.verify_rows(c, a["rows"], a)          # the model's own rows and outcomes: `verify` raises nothing
        undecidable[c.id] = int(flags.sum())
        RF.STATS["cases"][c.id]["undecidable"] = undecidable[c.id]
        assert undecidable[c.id] <= 0.01 * c.scn.n, (undecidable[c.id], c.context())     # the cap of test_gpu_spending_rule.py
    t3 = time.time()
    stats = RF.STATS["cases"]
    print(f"rule_fuzz, count_fuzz seed {F.seed()}: {len(cases)} cases, {sum(c.scn.n for c in cases)} paths; calibration {t1 - t0:.1f} s "
          f"(0.0 if another test made the cases; per class {RF.STATS['seconds']}), the model's answers {t2 - t1:.1f} s, verify {t3 - t2:.1f} s")
    for c in cases:
        print(f"  {c.id}: {stats[c.id]}")
    mixed = [c.id for c in cases if F.MIXED[0] * c.scn.n <= stats[c.id]["failed"] <= F.MIXED[1] * c.scn.n]
    raised = [c.id for c in cases if stats[c.id]["raised"] > 0]
    floor = [c.id for c in cases if c.rule[4] < 1.0 and stats[c.id]["floor"] > 0]
    cut = [c.id for c in cases if stats[c.id]["cut"] >= 0.05 * stats[c.id]["begun"] and stats[c.id]["begun"] > 0]
    pre = {c.id: stats[c.id]["pre_retirement"] for c in cases if stats[c.id]["pre_retirement"] > 0}
    print(f"  mixed {len(mixed)}, with raised path-years {len(raised)}, at a floor below 1 {len(floor)}, >= 5 % of begun path-years cut {len(cut)}, "
          f"paths failing before retirement {pre}, undecidable paths {sum(undecidable.values())} of {sum(c.scn.n for c in cases)}")
    assert len(mixed) >= 30, sorted(set(stats) - set(mixed))
    assert len(raised) >= 10, raised
    assert len(floor) >= 15, floor
    assert len(cut) >= 25, cut
    pinned = [c for c in cases if c.rname == "pinned"]
    assert len(pinned) >= 6
    for c in pinned:
        rows = answers[c.id]["rows"]
        assert stats[c.id]["cut"] == 0 and stats[c.id]["raised"] == 0 and np.all((rows == 1.0) | np.isnan(rows)), c.context()
    assert pre, "no case has a path with years_to_ruin == 0.0"
    for c in cases:                                      # a path that fails before retirement begins no year: the rule stays inert
        a = answers[c.id]
        assert np.all(np.isnan(a["rows"][:, a["years_to_ruin"] == 0.0])), c.context()
    # every case keeps its plan: the plan of count_fuzz but for the level, its path range included
    for cls in RF.CLASSES:
        for c, s in zip(RF.cases(oracle, cls), F.scenarios(oracle, cls)):
            assert (c.scn.wm, c.scn.seed, c.scn.stream, c.scn.begin, c.scn.n) == (s.wm, s.seed, s.stream, s.begin, s.n) and c.scn.n == F.PATHS[s.index % 2]
            assert {k: v for k, v in c.scn.cfgd.items() if k != "monthly_expenses"} == {k: v for k, v in s.cfgd.items() if k != "monthly_expenses"}
            assert F.CAL_LO <= c.level <= F.CAL_HI and c.scn.cfgd["monthly_expenses"] == c.level
    begins = {c.scn.begin for c in cases}
    assert begins == {0, 2 ** 32 - 100, 2 ** 40}, begins
    assert {c.rname for c in cases} == set(RF.RULES) and {c.scn.stream for c in cases} == {0, 1}


def test_the_tie_cases_tie_exactly_and_keep_the_multiplier(oracle):
    """Every year of every path of `rule_fuzz.tie_cases`: the oracle's real balance IS r0, bit for bit, so under `always` the
    decision is neither a cut nor a raise; the model keeps m = 1 and `verify`, whose tolerance straddles the tie, calls every
    path undecidable (which is why the GPU test holds these cases to the model's rows and not to `verify`)."""
    for c in RF.tie_cases(oracle):
        a = RF.answer(oracle, c)
        ry = RF.TIE_YEARS
        assert a["rows"].shape == (ry, RF.TIE_PATHS) and np.all(a["rows"] == 1.0) and a["success"].all(), c.context()
        assert a["year_counts"].tolist() == [[RF.TIE_PATHS, 0, 0, 0]] * ry, c.context()
        for run in a["runs"][:3] + a["runs"][-1:]:
            r0 = float(run["start_balance"][0]) / float(run["inflation_at_retirement"][0])
            real = run["real_trajectory"][-ry:, 0]
            assert r0 > 250_000.0 - 1.0 and np.all(real == r0) and np.all(run["trajectory"][-ry:, 0] == r0), c.context()
        assert RF.verify_rows(c, a["rows"], a).all(), c.context()


def test_the_levels_do_not_depend_on_the_order_of_generation(oracle):
    """Generating a class twice gives the same levels (the GPU tests generate class by class)."""
    again = RF._generate(oracle, "mask1", 2)
    assert [(c.id, c.level) for c in again] == [(c.id, c.level) for c in RF.cases(oracle, "mask1")[:2]]
