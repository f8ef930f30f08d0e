"""Shared pieces of the glide whole-path launch tests (tests/test_gpu_glide_run*.py).

The model of a glide path (tests/glide_model.cpp) keeps the per-path columns and the three yearly trajectories but none of the
launch's integers; `integers` forms them from those columns the way the oracle's batch loop does (oracle/mcr_oracle.c: the
counters, `wr_df.count(axis=1)`, and the ruin bin: 0 for a failure before retirement, 1 + the retirement year of a failure inside
it, ry + 1 for a failure of the terminal settlement).  `years_to_ruin` alone cannot tell a failure in the last month of the last
year from a failure of the settlement behind it (both are `ry`): the first leaves the last withdrawal rate NaN, the second does
not.  tests/test_glide_run_cpu.py holds `integers` to the oracle's own integers."""

from __future__ import annotations

import numpy as np

from monte_carlo_retirement_amd import engine as E

BLOCKS = ("counters", "wr_obs_counts", "ruin_year_bins", "trajectory_bins", "real_trajectory_bins", "wr_bins", "final_success_bins")
INTEGERS = BLOCKS[:3]
COLUMNS = E.SUMMARY_FIELDS + ("success",)


def integers(run, ry: int) -> dict:
    """`counters`, `wr_obs_counts` and `ruin_year_bins` of a run given by its per-path columns and withdrawal-rate rows."""
    ok = run["success"].astype(bool)
    wr = run["withdrawal_rate_trajectory"]
    ytr = run["years_to_ruin"]
    bins = np.zeros(ry + 2, dtype=np.uint64)
    failed = ~np.isnan(ytr)
    assert np.array_equal(failed, ~ok)
    month = np.rint(ytr[failed] * 12.0).astype(np.int64)
    settlement = (month == 12 * ry) & ~np.isnan(wr[ry - 1][failed])
    which = np.where(month == 0, 0, np.where(settlement, ry + 1, 1 + (np.maximum(month, 1) - 1) // 12))
    np.add.at(bins, which, 1)
    return {"counters": np.array([int(ok.sum()), ok.size], dtype=np.uint64),
            "wr_obs_counts": np.count_nonzero(~np.isnan(wr), axis=1).astype(np.uint64), "ruin_year_bins": bins}


def with_integers(run, ry: int) -> dict:
    return dict(run, **integers(run, ry))


def row_start(wm: int) -> int:
    return wm // 12 + (1 if wm % 12 else 0)         # the sample at retirement: row num_working_years


def same_bits(a, b) -> bool:
    """Equal bit for bit, NaNs included (one NaN pattern: the library stores 0x7ff8...)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_identities(yb, summ, n: int, wm: int, what=""):
    """The internal identities of one yearly-bins launch, and its two rows that a summary launch over the same paths gives exactly."""
    import bin_rule

    assert np.all(yb["trajectory_bins"].sum(axis=1) == n) and np.all(yb["real_trajectory_bins"].sum(axis=1) == n), what
    assert np.array_equal(yb["wr_bins"].sum(axis=1), yb["wr_obs_counts"]), what
    ok = summ["success"].astype(bool)
    assert int(yb["final_success_bins"].sum()) == int(yb["counters"][0]) == int(ok.sum()) and int(yb["counters"][1]) == n, what
    assert np.array_equal(yb["final_success_bins"].astype(np.int64), bin_rule.cells(summ["final_balance"][ok], yb["edges"])), what
    assert np.array_equal(yb["trajectory_bins"][row_start(wm)].astype(np.int64), bin_rule.cells(summ["start_balance"], yb["edges"])), what
    for k in INTEGERS:
        assert yb[k].tolist() == summ[k].tolist(), (k, what)
