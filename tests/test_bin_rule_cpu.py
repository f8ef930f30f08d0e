"""The yearly-table rule of tests/bin_rule.py and the comparison functions of tests/test_gpu_numpy_stream_vs_oracle.py, with the
oracle alone (no device).

1.  What the edge at 0 gave away.  The rule the three call sites used counted an entry "near an edge" when it was within 1e-8 of
    ANY edge; the default edges start at 0.0, and failed paths' balances and years without a withdrawal are exactly 0.0.  With
    the suite's seed, on the 68 plans' Philox runs and the default 256-bin edges, the three yearly tables have 5 073 rows of
    2 020 067 entries; 266 768 entries counted as near an edge, every one an exact zero, none within 1e-8 of any other edge;
    1 685 rows carried an allowance of twice their number of zeros.  Under the rule of tests/bin_rule.py the allowance is 0 on
    every row of every plan: on these plans the yearly-table comparison is cell for cell exact.  The same on the NumPy leg and
    the three history schemes, where the allowance left is printed and capped at 1 % of a row's entries.

2.  The comparisons can fail.  The oracle's own run passes `same_summary`, `same_full_output` and `same_year_bins`; a copy with one
    value error that leaves every flag and integer alone is rejected.  The last error, three entries of a row moved from one
    interior bin to its neighbour, passes the OLD rule wherever the row has three exact zeros and fails the new one on every
    plan."""

from __future__ import annotations

import time

import numpy as np

import bin_rule
import count_fuzz as F
import history_fuzz as HF
import history_scheme_fuzz as SF
from monte_carlo_retirement_amd import engine as E

BLOCK = 12                                       # the block length of tests/test_gpu_history_stream.py and test_gpu_history_schemes.py
YEARLY = (("trajectory", "edges"), ("real_trajectory", "edges"), ("withdrawal_rate_trajectory", "wr_edges"))
CAP = 0.01                                       # legs other than Philox: the allowance left, as a share of a row's entries


def _legs(O):
    """leg -> (the plans, the oracle's trajectory run of a plan or None where the leg leaves the plan out for its money scale)."""
    plans = [s for cls in F.CLASSES for s in F.scenarios(O, cls)]
    table = HF.synthetic_record()

    def usable(run):
        return run if F.money_scale(run) < F.SCALE_LIMIT else None

    return {
        "Philox": (plans, lambda s: F.oracle_run(O, s, trajectories=True)),
        "NumPy": (plans + F.numpy_extra(O), lambda s: F.oracle_run_numpy(O, s, trajectories=True)),
        "history, block": (plans, lambda s: usable(HF.oracle_run_history(O, s, table, BLOCK))),
        "history, stationary": (plans, lambda s: usable(SF.oracle_run_scheme(O, s, table, BLOCK, SF.STATIONARY))),
        "history, cohorts": (plans, lambda s: usable(SF.oracle_run_scheme(O, s, table, BLOCK, SF.COHORTS))),
    }


def _figures(plans, run_of):
    """The allowance figures of one leg over the three yearly tables and the default edges, and its worst row."""
    edges = {"edges": E.default_year_edges(), "wr_edges": E.default_wr_edges()}
    fig = {"plans": 0, "rows": 0, "entries": 0, "old_near": 0, "zeros": 0, "old_rows": 0, "new_near": 0, "new_rows": 0, "negative": 0, "above_wr": 0}
    worst = (0.0, None)
    for s in plans:
        run = run_of(s)
        if run is None:
            continue
        fig["plans"] += 1
        for key, which in YEARLY:
            e = edges[which]
            for t, row in enumerate(run[key]):
                row = row[~np.isnan(row)]
                old, new = bin_rule.old_near(row, e), bin_rule.near_an_edge(row, e)
                zeros = int(np.count_nonzero(row == 0.0))
                assert old == zeros + new, (key, t, old, zeros, new, s.context("the old allowance is the zeros and the entries near another edge"))
                fig["rows"] += 1
                fig["entries"] += row.size
                fig["old_near"] += old
                fig["zeros"] += zeros
                fig["old_rows"] += old > 0
                fig["new_near"] += new
                fig["new_rows"] += new > 0
                fig["negative"] += int(np.count_nonzero(row < 0.0))
                if which == "wr_edges":
                    fig["above_wr"] += int(np.count_nonzero(row > e[-1]))
                if new and 2 * new / row.size > worst[0]:
                    worst = (2 * new / row.size, (s.cls, s.index, key, t, new, row.size))
    return fig, worst


def test_the_edge_at_zero_was_the_whole_allowance(oracle):
    t0 = time.time()
    legs = _legs(oracle)
    for leg, (plans, run_of) in legs.items():
        fig, worst = _figures(plans, run_of)
        print(f"{leg} ({time.time() - t0:.1f} s): {fig['plans']} plans, {fig['rows']} rows hold {fig['entries']} entries; old rule: {fig['old_near']} entries "
              f"near an edge, {fig['zeros']} of them exact zeros, {fig['old_rows']} rows with an allowance; new rule: {fig['new_near']} entries near an "
              f"edge on {fig['new_rows']} rows, worst allowance / entries of a row {worst[0]:.4f} {worst[1]}; negative entries {fig['negative']}, "
              f"withdrawal rates above the top edge {fig['above_wr']}")
        assert fig["negative"] == 0, leg                       # nothing lies below the edge at 0: cell 0 of every row is 0
        assert fig["old_near"] == fig["zeros"] + fig["new_near"], leg
        if leg == "Philox":
            assert fig["plans"] == 68 and fig["old_near"] == fig["zeros"] > 0 and fig["old_rows"] > 0, fig
            assert fig["new_near"] == 0 and fig["new_rows"] == 0, (fig, worst)      # cell for cell exact on these plans
        else:
            assert fig["plans"] >= 65, (leg, fig)
            assert worst[0] <= CAP, (leg, worst)


# ---- 2. the comparisons can fail --------------------------------------------------------------------------------------------------
def _old_rule_passes(got, row, edges) -> bool:
    """The rule as the three call sites had it, with the edge at 0 counted."""
    row = row[~np.isnan(row)]
    exp = bin_rule.cells(row, edges)
    got = np.asarray(got).astype(np.int64)
    return int(got.sum()) == row.size and int(np.abs(got - exp).sum()) <= 2 * bin_rule.old_near(row, edges)


def _rejects(check, scn, got, ora) -> bool:
    try:
        check(scn, got, ora)
    except AssertionError:
        return True
    return False


def _copy(run, **changed):
    return dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in run.items()}, **changed)


def _move_three(year, ora):
    """A copy of the `year` launch with 3 entries of one trajectory_bins row moved from an interior bin to its upper neighbour:
    the row with the most exact zeros among those that have an interior bin of 3 entries.  Returns (copy, row index, its zeros)."""
    table = year["trajectory_bins"]
    nb = table.shape[1] - 2
    best = None
    for t in range(table.shape[0]):
        cells = np.nonzero(table[t, 2:nb] >= 3)[0]          # cells 2 .. nb - 1: bins 1 .. nb - 2, whose upper neighbour is a bin too
        if cells.size:
            zeros = int(np.count_nonzero(ora["trajectory"][t] == 0.0))
            if best is None or zeros > best[2]:
                best = (t, 2 + int(cells[0]), zeros)
    assert best is not None, "no row with three entries in an interior bin"
    t, c, zeros = best
    moved = table.copy()
    moved[t, c] -= 3
    moved[t, c + 1] += 3
    return dict(year, trajectory_bins=moved), t, zeros


def test_the_comparisons_reject_a_value_error_that_leaves_the_flags_alone(oracle):
    import test_gpu_numpy_stream_vs_oracle as T
    from test_count_fuzz_cpu import _as_launches

    ctx = lambda scn, route: scn.context(route + " (the oracle standing in for the Philox launch)")     # noqa: E731
    summary = lambda s, g, o: T.same_summary(s, g, o, ctx=ctx)        # noqa: E731
    full = lambda s, g, o: T.same_full_output(s, g, o, ctx=ctx)       # noqa: E731
    year = lambda s, g, o: T.same_year_bins(s, g, o, ctx=ctx)         # noqa: E731
    t0 = time.time()
    rejected, applies = {}, {}
    old_passes = new_fails = plans = 0

    def note(what, check_name, check, scn, got, ora, holds=True):
        """Count the plans error `what` applies to (`holds`) and those on which `check` rejects it."""
        applies[what, check_name] = applies.get((what, check_name), 0) + bool(holds)
        if holds:
            rejected[what, check_name] = rejected.get((what, check_name), 0) + _rejects(check, scn, got, ora)

    for cls in F.CLASSES:
        for scn in F.scenarios(oracle, cls)[:3]:
            plans += 1
            ora = F.oracle_run(oracle, scn, trajectories=True)
            own = _as_launches(ora)
            summary(scn, own["summary"], ora)                       # the oracle's own run passes every comparison
            full(scn, own["full"], ora)
            year(scn, own["year"], ora)
            traj, real, wr = ora["trajectory"], ora["real_trajectory"], ora["withdrawal_rate_trajectory"]
            scale = np.maximum(1.0, np.abs(traj).max(axis=0))
            i = int(np.argmax(scale))
            assert scale[i] > 1e3, scn.context()                    # (1e-8 of it is then outside ABS + REL x scale = 1e-6 + 1e-9 x scale)
            # a. a summary field off by 1e-8 of the path's money scale on one path
            for key in T.SUMMARY:
                bad = _copy(ora)
                bad[key][i] += 1e-8 * scale[i]
                note(f"{key} off by 1e-8 of the scale", "summary", summary, scn, bad, ora)
                note(f"{key} off by 1e-8 of the scale", "full", full, scn, bad, ora)
            # b. the trajectory rows shifted by one year
            bad = _copy(ora, trajectory=np.concatenate([traj[1:], traj[-1:]]))
            note("trajectory rows shifted by one year", "full", full, scn, bad, ora)
            note("trajectory rows shifted by one year", "year", year, scn, _as_launches(bad)["year"], ora)
            # c. the real trajectory deflated by the NEXT year's price level (level = nominal / real where there is money)
            with np.errstate(divide="ignore", invalid="ignore"):
                level = np.where(real != 0.0, traj / real, np.nan)
                after = np.concatenate([level[1:], level[-1:]])
                deflated = np.where(np.isfinite(after) & (real != 0.0), traj / after, real)
            inflates = scn.cfgd["inflation_rate_mean"] != 0.0 or scn.cfgd["inflation_rate_volatility"] != 0.0
            bad = _copy(ora, real_trajectory=deflated)
            note("real trajectory deflated by the next year's level", "full", full, scn, bad, ora, inflates)
            note("real trajectory deflated by the next year's level", "year", year, scn, _as_launches(bad)["year"], ora, inflates)
            # d. first_year_gross_withdrawal and its real twin swapped (the same number for a plan that retires at once)
            a, b = "first_year_gross_withdrawal", "first_year_real_gross_withdrawal"
            differ = bool(np.any(np.abs(ora[a] - ora[b]) > 1e-6 + 1e-8 * scale))
            bad = _copy(ora, **{a: ora[b].copy(), b: ora[a].copy()})
            note("first-year withdrawal and its real twin swapped", "summary", summary, scn, bad, ora, differ)
            note("first-year withdrawal and its real twin swapped", "full", full, scn, bad, ora, differ)
            # e. one withdrawal rate turned NaN
            seen = np.argwhere(~np.isnan(wr))
            bad = _copy(ora)
            if seen.size:
                bad["withdrawal_rate_trajectory"][tuple(seen[len(seen) // 2])] = np.nan
            note("one withdrawal rate turned NaN", "full", full, scn, bad, ora, seen.size > 0)
            note("one withdrawal rate turned NaN", "year", year, scn, _as_launches(bad)["year"], ora, seen.size > 0)
            # f. three entries of a row that has exact zeros moved from one interior bin to its neighbour
            moved, t, zeros = _move_three(own["year"], ora)
            old_ok = _old_rule_passes(moved["trajectory_bins"][t], traj[t], moved["edges"])
            assert old_ok == (zeros >= 3), (t, zeros, scn.context("the old rule"))
            old_passes += old_ok
            new_fails += _rejects(year, scn, moved, ora)
    print(f"catch check ({time.time() - t0:.1f} s), the first three plans of each class ({plans} plans): plans rejected / plans the error applies to")
    for (what, name), n in sorted(applies.items()):
        print(f"  {what}: {name}: {rejected.get((what, name), 0)} / {n}")
        assert rejected.get((what, name), 0) == n, (what, name, rejected.get((what, name), 0), n)
        assert n >= (plans if "off by" in what or "shifted" in what or "NaN" in what else plans // 2), (what, name, n)
    print(f"  three entries moved to the neighbouring bin: the old rule passes on {old_passes} of {plans} plans, the new rule fails on {new_fails}")
    assert old_passes >= 1 and new_fails == plans, (old_passes, new_fails, plans)
