"""The split re-run of a screened launch with its consumer wave restated in pairs of months on an event row (csrc/mcr_events.h,
path_kernel's "PAIRS"): counts bit for bit.

Every launch runs under MCR_K1_SCREEN=1 in both forms of the split re-run (MCR_K1_RERUN_PRODUCERS=1: the 256-path workgroup,
=2: one consumer and two producer waves on 64 paths) against the classic route (MCR_K1_SCREEN=0); `counters`, `wr_obs_counts`
and `ruin_year_bins` must be equal bit for bit, and for config.json equal to the CPU oracle's.  Shapes: 300 and 4096 paths,
4096 paths across 2^32, 4096 paths from 5 10^9.

The plans are chosen for what the restated bookkeeping can get wrong (PLANS below names, per plan, the rows): working_months
even and odd, total_months % 4 = 0 .. 3, windows that open and close on even and on odd rows, a window edge on a year boundary,
on the retirement boundary and on a priority-threshold row (total_months / 2, 3/4, 9/10 of it), one and two income records,
and the nearly-all-doubtful plan in which lanes die and workgroups vote themselves dead.  `test_plans_show_what_they_are_for`
checks those rows on the CPU side of the library (engine.stream_start_month_index), so a plan cannot drift off its purpose.

`monthly_expenses` of a plan is chosen on the CPU with tests/screen_model.py: the lowest step of a ladder (x 1.25 a step from the
plan's own) at which half of a 128-path sample is DOUBTFUL in the model.  The re-run must never be empty: on every shape the
screening kernel's own classes (engine.screen_paths) must call at least a quarter of the paths doubtful.
"""

from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

SEED, STREAM = 12345, 1
COUNT_KEYS = ("counters", "wr_obs_counts", "ruin_year_bins")
KNOBS = ("MCR_K1_SCREEN", "MCR_K1_SCREEN_MIN_PATHS", "MCR_K1_SCREEN_EXPECTED", "MCR_K1_RERUN_PRODUCERS", "MCR_K1_SPLIT_MAX_WAVES",
         "MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS", "MCR_K1_SEGMENT_ORDER", "MCR_K1_GROWTH_FORM",
         "MCR_K1_MONTH_FORM", "MCR_K1_STREAM_FORM")
FORMS = {"256-path form": {"MCR_K1_RERUN_PRODUCERS": "1"}, "64-path form": {"MCR_K1_RERUN_PRODUCERS": "2"}}
SAMPLE, LADDER, LADDER_STEPS = 128, 1.25, 16
AGE = 40.0


def _config(**over):
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        return dict(json.load(fh), **over)


def _record(open_row, years, amount=3000.0, tax=0.2):
    """An indexed record whose window opens on row `open_row` of the path (row 0 = the first accumulation month)."""
    return {"name": f"opens at row {open_row}", "monthly_amount_today": amount, "start_at_age": AGE + open_row / 12.0,
            "duration_years": years, "inflation_indexed": True, "tax_rate": tax}


def _short(wm, records):
    # (the ladder starts low: at the chosen level about half of the paths are SAFE, and the doubtful ones both succeed and fail,
    # so a window a month off its rows changes the counts)
    return _config(retirement_years=20, initial_balance=1.5e6, monthly_expenses=1000.0, other_income_streams=records), wm


# name: (config, working_months, [(open row, close row or None)] the plan is built to show, choose the expenses?)
# 20-year plans: total_months = wm + 240; the priority falls on rows total // 2, 3 total // 4, 9 total // 10
PLANS = {
    # wm odd, total 833 (% 4 = 1); the pension opens at 65: row 300, even, and never closes
    "config wm233": (_config(), 233, [(300, None)], True),
    # lanes die, workgroups vote themselves dead
    "nearly all doubtful": (_config(monthly_expenses=40000.0), 233, [(300, None)], False),
    # wm even, total 264 (% 4 = 0), thresholds 132 198 237: opens ON threshold 132 (even), closes on 192 (even, a plan-year
    # boundary); the second record opens on the retirement boundary (row 24) and never closes
    "wm24 two records": (*_short(24, [_record(132, 5), _record(24, None, amount=1500.0, tax=0.1)]), [(132, 192), (24, None)], True),
    # wm odd, total 265 (% 4 = 1): one record, opens on 37 (odd; the first retirement-year boundary), closes on 61 (odd)
    "wm25 one record": (*_short(25, [_record(37, 2)]), [(37, 61)], True),
    # wm even, total 266 (% 4 = 2), thresholds 133 199 239: opens on 36 (even, a plan-year boundary), closes on 48; the second
    # opens ON threshold 199 (odd) and never closes
    "wm26 two records": (*_short(26, [_record(36, 1), _record(199, None, amount=2000.0)]), [(36, 48), (199, None)], True),
    # wm odd, total 267 (% 4 = 3), thresholds 133 200 240: opens on the retirement boundary (row 27, odd), closes on 147 (odd); the
    # second opens ON threshold 240 (even) and closes on 264 (even)
    "wm27 two records": (*_short(27, [_record(27, 10), _record(240, 2, amount=2000.0)]), [(27, 147), (240, 264)], True),
}
SIZES = {"300": (0, 300), "4096": (0, 4096), "4096 across 2^32": (2**32 - 2048, 4096), "4096 from 5e9": (5 * 10**9, 4096)}


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _expenses(plan):
    """The plan's monthly_expenses: its own, or the lowest ladder step at which half of the model's sample is DOUBTFUL."""
    import screen_model

    cfgd, wm, _, choose = PLANS[plan]
    level = float(cfgd["monthly_expenses"])
    if not choose:
        return level
    for _ in range(LADDER_STEPS):
        c = dict(cfgd, monthly_expenses=level)
        safe = screen_model.model(params_from_config(Config(**c)), c, wm, SEED, STREAM, 0, SAMPLE)["safe"]
        if 2 * int((~safe).sum()) >= SAMPLE:
            return level
        level *= LADDER
    raise AssertionError(f"{plan}: no ladder step makes half of the sample doubtful")


def _plan(plan):
    cfgd, wm, rows, _ = PLANS[plan]
    cfgd = dict(cfgd, monthly_expenses=_expenses(plan))
    return cfgd, params_from_config(Config(**cfgd)), wm, rows


def _ints(r):
    return np.concatenate([np.asarray(r[k]).astype(np.int64) for k in COUNT_KEYS])


@functools.lru_cache(maxsize=None)
def _oracle(plan, begin, n):
    from oracle import oracle as O

    _, p, wm, _ = _plan(plan)
    return _ints(O.run_batch(p, SEED, STREAM, begin, n, wm, want_summary=False, want_trajectories=False))


def test_plans_show_what_they_are_for():
    seen = {"wm parity": set(), "total % 4": set(), "open parity": set(), "close parity": set(), "records": set()}
    edges = set()
    for plan in PLANS:
        cfgd, p, wm, rows = _plan(plan)
        total = wm + 12 * int(cfgd["retirement_years"])
        kept = [cfgd["other_income_streams"][i] for i, _ in E.kept_streams(p, wm)]
        assert len(kept) == len(rows), plan
        seen["wm parity"].add(wm & 1); seen["total % 4"].add(total % 4); seen["records"].add(len(kept))
        for rec, (first, close) in zip(kept, rows):
            assert wm + E.stream_start_month_index(float(cfgd["current_age"]), wm, float(rec["start_at_age"])) == first, (plan, rec)
            assert (close is None) == (rec["duration_years"] is None) and (close is None or close == first + 12 * rec["duration_years"]), (plan, rec)
            seen["open parity"].add(first & 1)
            for row in (first, close):
                if row is None:
                    continue
                if row is close:
                    seen["close parity"].add(row & 1)
                edges |= {name for name, holds in (("plan-year boundary", row % 12 == 0), ("retirement-year boundary", row > wm and (row - wm) % 12 == 0),
                                                    ("retirement boundary", row == wm), ("priority threshold", row in (total // 2, 3 * total // 4, 9 * total // 10))) if holds}
    assert seen == {"wm parity": {0, 1}, "total % 4": {0, 1, 2, 3}, "open parity": {0, 1}, "close parity": {0, 1}, "records": {1, 2}}, seen
    assert edges == {"plan-year boundary", "retirement-year boundary", "retirement boundary", "priority threshold"}, edges


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("plan", list(PLANS))
def test_paired_rerun_counts_equal_the_classic_route_bit_for_bit(plan, size):
    begin, n = SIZES[size]
    _, p, wm, _ = _plan(plan)
    assert _with_env({}, lambda: E.screen(p, wm, 10**6)), plan             # the plan qualifies: MCR_K1_SCREEN=1 takes the route
    cls = _with_env({}, lambda: E.screen_paths(p, SEED, STREAM, begin, n, wm))["cls"]
    doubtful = int((cls == 1).sum())
    assert 4 * doubtful >= n, (plan, size, doubtful)                       # the re-run is never empty
    run = lambda env: _ints(_with_env(env, lambda: E.run_batch_host(p, SEED, STREAM, begin, n, wm, want_summary=False, want_trajectories=False)))  # noqa: E731
    classic = run({"MCR_K1_SCREEN": "0"})
    assert int(classic[1]) == n
    print(f"  {plan} / {size}: monthly_expenses {_expenses(plan):.2f}, {doubtful} of {n} paths doubtful in the screening kernel, {int(classic[0])} succeed")
    if plan == "config wm233":
        want = _oracle(plan, begin, n)
        assert np.array_equal(classic, want), (plan, size, "classic route vs oracle", np.nonzero(classic != want)[0][:8].tolist())
    if plan == "nearly all doubtful":
        assert int(classic[0]) * 64 < n, (plan, int(classic[0]))            # whole 64-path workgroups die
    for name, env in FORMS.items():
        got = run(dict(env, MCR_K1_SCREEN="1"))
        assert np.array_equal(got, classic), (plan, size, name, np.nonzero(got != classic)[0][:8].tolist(), got[:2].tolist(), classic[:2].tolist())
