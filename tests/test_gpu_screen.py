"""The SCREENED route of a count-only launch (csrc/mcr_screen.h, screen_kernel and path_kernel's LIST form; DESIGN.md "screened
count-only launches").

Same results: every launch runs with MCR_K1_SCREEN=1 (screening kernel + fp64 re-run of the doubtful paths, in both forms of
the re-run) against MCR_K1_SCREEN=0 (the classic kernels); counters, wr_obs_counts and ruin_year_bins must be equal bit for
bit, and equal to the CPU oracle's.

Classification: the screening kernel alone (mcr_screen_paths_rng) over 4096 paths of three plans.  (a) every path it calls
SAFE succeeds in the oracle with no ruin year; (b) its fp32 final total is within 1e-2 of the oracle's final balance (the design
tolerates 0.95, a factor of 24 on the capacity; the expected deviation is about 1e-5); (c) it calls at most 8 % of config.json's
paths doubtful, so the test cannot pass on an empty SAFE set.  Observed on MI355X (LABNOTES R24): see the table there.

Plans with income records and random markets (20-60 % volatility, rho = +-1, rates near 1, contribution growth, odd month
counts), and the kernel's per-path `min_ratio` and `final_total` held to an fp64 restatement of its month rather than to the
oracle's final balance alone: tests/test_gpu_screen_vs_oracle.py."""

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
KNOBS = ("MCR_K1_SCREEN", "MCR_K1_SCREEN_MIN_PATHS", "MCR_K1_SCREEN_EXPECTED", "MCR_K1_SPLIT_MAX_WAVES", "MCR_K1_SEGMENTS",
         "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS", "MCR_K1_SEGMENT_ORDER", "MCR_K1_GROWTH_FORM", "MCR_K1_MONTH_FORM",
         "MCR_K1_STREAM_FORM")
UNSPLIT = {"MCR_K1_SCREEN_EXPECTED": "1e6"}      # n x expected / 64 wavefronts is then beyond any split limit: the unsplit LIST kernel


def _config(name="config.json", **over):
    with open(os.path.join(REPO, "scenarios", name)) as fh:
        return dict(json.load(fh), **over)


def _stream(amount, start, years=None, tax=0.2):
    return {"name": f"s{amount}", "monthly_amount_today": amount, "start_at_age": start, "duration_years": years,
            "inflation_indexed": True, "tax_rate": tax}


#         name                    config                                                                                      wm
PLANS = {
    "config wm233":              (_config(),                                                                                  233),
    "config wm7":                (_config(),                                                                                  7),
    "all safe":                  (_config(initial_balance=1.0e9),                                                             233),
    "nearly all doubtful":       (_config(monthly_expenses=40000.0),                                                          233),
    "jorge rho 0.3 wm75":        (_config("jorge.json", equity_inflation_correlation=0.3),                                    75),
    "S60":                       (_config(initial_balance=2.0e6, inv1_returns_volatility=0.15, equity_inflation_correlation=0.3), 120),
    # retirement begins at 40 + 233 / 12 = 59.4: both windows open inside it, the second one closes inside it too
    "two records open inside":   (_config(other_income_streams=[_stream(3000.0, 63.0, tax=0.275), _stream(2500.0, 70.5, years=12, tax=0.1)]), 233),
}
#         name                  first path      paths
SIZES = {
    "300":                      (0,             300),           # one full workgroup and a partial one
    "257":                      (0,             257),
    "64x17+1":                  (0,             64 * 17 + 1),
    "straddles 2^32":           (2**32 - 100,   300),
    "begins at 5e9":            (5 * 10**9,     300),
}


def _params(plan):
    cfgd, wm = PLANS[plan]
    return params_from_config(Config(**cfgd)), wm


@functools.lru_cache(maxsize=None)
def _oracle(plan, begin, n, summary=False):
    from oracle import oracle as O

    p, wm = _params(plan)
    return O.run_batch(p, SEED, STREAM, begin, n, wm, want_summary=summary, want_trajectories=False)


def _run(p, wm, begin, n, env):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return E.run_batch_host(p, SEED, STREAM, begin, n, wm, want_summary=False, want_trajectories=False)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _ints(r):
    return np.concatenate([np.asarray(r[k]).astype(np.int64) for k in COUNT_KEYS])


def _check(plan, begin, n, envs):
    p, wm = _params(plan)
    want = _ints(_oracle(plan, begin, n))
    classic = _ints(_run(p, wm, begin, n, {"MCR_K1_SCREEN": "0"}))
    assert int(classic[1]) == n
    assert np.array_equal(classic, want), (plan, "classic vs oracle", np.nonzero(classic != want)[0][:8].tolist())
    for env in envs:
        got = _ints(_run(p, wm, begin, n, dict(env, MCR_K1_SCREEN="1")))
        assert np.array_equal(got, classic), (plan, env, np.nonzero(got != classic)[0][:8].tolist(), got[:2].tolist(), classic[:2].tolist())
    return classic


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("plan", list(PLANS))
def test_screened_counts_equal_the_classic_kernels_and_the_oracle(plan, size):
    begin, n = SIZES[size]
    p, wm = _params(plan)
    assert E.screen(p, wm, 10**6)                      # the plan qualifies: MCR_K1_SCREEN=1 takes the route
    c = _check(plan, begin, n, ({}, UNSPLIT))          # the re-run in its producer / consumer form and in its unsplit form
    if plan == "all safe":
        assert int(c[0]) == n
    if plan == "nearly all doubtful":
        assert 10 * int(c[0]) < n                      # the oracle's success share is below 10 %: the list is nearly full


def test_a_larger_launch_with_the_unsplit_rerun():
    """20 000 paths: 79 workgroups of the screening kernel, and a list long enough to span several of the re-run's."""
    _check("config wm233", 777, 20000, (UNSPLIT, {}))


# ---- classification -------------------------------------------------------------------------------------------------
N_CLS = 4096
CLS_PLANS = {"config wm233": 0.08, "S60": None, "nearly all doubtful": None}      # (c): the largest doubtful share allowed


@pytest.mark.parametrize("plan", list(CLS_PLANS))
def test_what_the_screening_kernel_calls_safe_is_safe(plan):
    p, wm = _params(plan)
    ref = _oracle(plan, 0, N_CLS, True)
    s = E.screen_paths(p, SEED, STREAM, 0, N_CLS, wm)
    safe = s["cls"] == 0
    assert set(np.unique(s["cls"]).tolist()) <= {0, 1}
    share = 1.0 - safe.mean()
    dev = np.abs(s["final_total"][safe].astype(np.float64) / ref["final_balance"][safe] - 1.0) if safe.any() else np.zeros(0)
    low = float(s["min_ratio"][safe].min()) if safe.any() else float("inf")
    print(f"{plan}: doubtful {share:.4f}, SAFE {int(safe.sum())}, max |final_total / final_balance - 1| {dev.max() if dev.size else 0.0:.3e}, "
          f"lowest min_ratio among SAFE {low:.2f}")
    # (a) SAFE -> a success with no ruin year in the oracle
    assert np.all(ref["success"][safe] == 1), np.nonzero(safe & (ref["success"] == 0))[0][:8].tolist()
    assert np.all(np.isnan(ref["years_to_ruin"][safe]))
    # (b) the fp32 path ends where the fp64 path ends
    assert dev.size == 0 or dev.max() <= 1e-2, dev.max()
    # every SAFE path kept the margin it was classified by
    assert low >= 24.0 * (1.0 - 1e-5)         # (cap x rcp(need) against cap >= 24 need: an fp32 rounding apart)
    # (c)
    if CLS_PLANS[plan] is not None:
        assert share <= CLS_PLANS[plan], share
    if plan == "nearly all doubtful":
        assert share > 0.9
