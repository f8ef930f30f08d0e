"""The forms of a screened launch's fp64 re-run (csrc/mcr_hip.hip, launch_screened; DESIGN.md "screened count-only launches"):
MCR_K1_RERUN_PRODUCERS=1, the 256-path producer / consumer workgroup; =2, one 64-path block per workgroup with one consumer and
two producer waves (path_kernel's NPROD = 2); and the unsplit LIST kernel (MCR_K1_SCREEN_EXPECTED=1e6).

Every case runs with MCR_K1_SCREEN=1 in the three forms and with MCR_K1_SCREEN=0 (the classic kernels); counters, wr_obs_counts
and ruin_year_bins must be equal bit for bit, and on config.json at working_months 233 equal to the CPU oracle's as well.

Sizes: 63, 64, 65 and 64 x 17 + 1 paths (a list shorter than, equal to and just past one 64-path block, and several blocks on
the full list), 300 paths across 2^32 (the producers' second Philox pass) and from 5 10^9.  Plans: total_months = working_months
+ 12 retirement_years, so working_months 232, 233, 234 and 235 are total_months = 0, 1, 2, 3 mod 4: the last pair of rows is
whole or ragged, and the last barrier belongs to producer 1's pair or to producer 0's."""

from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

pytestmark = pytest.mark.gpu

SEED, STREAM = 12345, 1
COUNT_KEYS = ("counters", "wr_obs_counts", "ruin_year_bins")
KNOBS = ("MCR_K1_SCREEN", "MCR_K1_SCREEN_MIN_PATHS", "MCR_K1_SCREEN_EXPECTED", "MCR_K1_RERUN_PRODUCERS", "MCR_K1_SPLIT_MAX_WAVES",
         "MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS", "MCR_K1_SEGMENT_ORDER", "MCR_K1_GROWTH_FORM",
         "MCR_K1_MONTH_FORM", "MCR_K1_STREAM_FORM")
FORMS = ({"MCR_K1_RERUN_PRODUCERS": "1"},
         {"MCR_K1_RERUN_PRODUCERS": "2"},
         {"MCR_K1_RERUN_PRODUCERS": "2", "MCR_K1_SCREEN_EXPECTED": "1e6"})     # (beyond any split limit: the unsplit LIST kernel)


def _config(**over):
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        return dict(json.load(fh), **over)


def _stream(amount, start, years=None, tax=0.2):
    return {"name": f"s{amount}", "monthly_amount_today": amount, "start_at_age": start, "duration_years": years,
            "inflation_indexed": True, "tax_rate": tax}


#         name                    config                                  working_months
PLANS = {
    "config wm233":              (_config(),                              233),      # total_months = 1 mod 4
    "config wm232":              (_config(),                              232),      # 0 mod 4
    "config wm234":              (_config(),                              234),      # 2 mod 4
    "config wm235":              (_config(),                              235),      # 3 mod 4
    "all safe":                  (_config(initial_balance=1.0e9),         233),      # an empty list: every workgroup returns
    "nearly all doubtful":       (_config(monthly_expenses=40000.0),      233),      # a full list
    # retirement begins at 40 + 233 / 12 = 59.4: both windows open inside it, the second one closes inside it too
    "two records open inside":   (_config(other_income_streams=[_stream(3000.0, 63.0, tax=0.275), _stream(2500.0, 70.5, years=12, tax=0.1)]), 233),
}
ORACLE_PLAN = "config wm233"
#         name                  first path      paths
SIZES = {
    "63":                       (0,             63),
    "64":                       (0,             64),
    "65":                       (0,             65),
    "64x17+1":                  (0,             64 * 17 + 1),
    "straddles 2^32":           (2**32 - 100,   300),
    "begins at 5e9":            (5 * 10**9,     300),
}


def _params(plan):
    cfgd, wm = PLANS[plan]
    return params_from_config(Config(**cfgd)), wm


@functools.lru_cache(maxsize=None)
def _oracle(plan, begin, n):
    from oracle import oracle as O

    p, wm = _params(plan)
    return O.run_batch(p, SEED, STREAM, begin, n, wm, want_summary=False, want_trajectories=False)


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


def _run(p, wm, begin, n, env):
    return _with_env(env, lambda: E.run_batch_host(p, SEED, STREAM, begin, n, wm, want_summary=False, want_trajectories=False))


def _ints(r):
    return np.concatenate([np.asarray(r[k]).astype(np.int64) for k in COUNT_KEYS])


def _check(plan, begin, n):
    p, wm = _params(plan)
    classic = _ints(_run(p, wm, begin, n, {"MCR_K1_SCREEN": "0"}))
    assert int(classic[1]) == n
    if plan == ORACLE_PLAN:
        want = _ints(_oracle(plan, begin, n))
        assert np.array_equal(classic, want), (plan, "classic vs oracle", np.nonzero(classic != want)[0][:8].tolist())
    for env in FORMS:
        got = _ints(_run(p, wm, begin, n, dict(env, MCR_K1_SCREEN="1")))
        assert np.array_equal(got, classic), (plan, env, np.nonzero(got != classic)[0][:8].tolist(), got[:2].tolist(), classic[:2].tolist())
    return classic


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("plan", list(PLANS))
def test_every_form_of_the_rerun_counts_what_the_classic_kernels_count(plan, size):
    begin, n = SIZES[size]
    p, wm = _params(plan)
    assert _with_env({}, lambda: E.screen(p, wm, 10**6))      # the plan qualifies: MCR_K1_SCREEN=1 takes the route
    c = _check(plan, begin, n)
    if plan == "all safe":
        assert int(c[0]) == n
    if plan == "nearly all doubtful":
        assert 10 * int(c[0]) < n                             # the success share is below 10 %: the list is nearly full


def test_a_launch_of_20000_paths():
    """A list of about 500 paths of 20 000: eight 64-path workgroups of 313 run, the others return."""
    _check(ORACLE_PLAN, 777, 20000)


def test_300_paths_are_not_screened_by_default_and_a_million_are():
    p, wm = _params(ORACLE_PLAN)
    assert not _with_env({}, lambda: E.screen(p, wm, 300))
    assert _with_env({}, lambda: E.screen(p, wm, 10**6))


@pytest.mark.parametrize("junk", ["0", "3", "two", "2 ", "12"])
def test_junk_in_the_knob_is_an_error(junk):
    p, wm = _params(ORACLE_PLAN)
    env = {"MCR_K1_SCREEN": "1", "MCR_K1_RERUN_PRODUCERS": junk}
    with pytest.raises(ValueError, match="MCR_K1_RERUN_PRODUCERS"):
        _with_env(env, lambda: E.screen(p, wm, 300))
    with pytest.raises(RuntimeError, match="MCR_K1_RERUN_PRODUCERS"):      # ... and the launch itself is refused (the engine's error type)
        _run(p, wm, 0, 300, env)
