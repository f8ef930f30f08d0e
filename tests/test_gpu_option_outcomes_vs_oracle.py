"""The income outcomes probe (`mcr_probe_income_outcomes_rng`) and `mcr_ruin_month_counts` against the CPU oracle, on the
stratified random plans of tests/count_fuzz.py and the five income options of tests/test_gpu_income_vs_oracle.py.

tests/test_gpu_option_outcomes.py compares the rows with summary launches of the same library; an error both share passes it.
Here the ORACLE's own per-path columns of a plan's five options are the reference, for every plan of every class: the NaN
pattern of both rows and `years_to_ruin` must equal them exactly, `final_balance` within the path contract of
tests/test_gpu_differential.py (``ABS + REL * max(|c|, the path's money scale)``, imported), and the ruin-month counts of the
GPU's rows must equal the counts of the oracle's columns.  Identical outcomes are demanded only below the 2^33 money scale,
so each oracle run's scale is asserted; no plan is waived."""

from __future__ import annotations

import numpy as np
import pytest

import count_fuzz as F
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from test_gpu_differential import ABS, REL
from test_gpu_income_vs_oracle import class_runs

pytestmark = pytest.mark.gpu
STREAM_FIELDS = ("monthly_amount_today", "start_at_age", "duration_years")


def oracle_rows(runs, k):
    """(final_balance where the path succeeds else NaN, years_to_ruin, the path's money scale), [5, n] each, of plan k."""
    mine = runs[5 * k: 5 * k + 5]
    fin = np.stack([np.where(np.asarray(r["success"]).astype(bool), r["final_balance"], np.nan) for r in mine])
    ruin = np.stack([np.asarray(r["years_to_ruin"], dtype=np.float64) for r in mine])
    scale = np.stack([np.maximum(1.0, np.abs(r["trajectory"]).max(axis=0)) for r in mine])
    return fin, ruin, scale


def month_counts(ruin, ry):
    out = np.zeros((ruin.shape[0], 12 * ry + 1), dtype=np.int64)
    for k, y in enumerate(ruin):
        out[k] = np.bincount(np.rint(12.0 * y[~np.isnan(y)]).astype(np.int64), minlength=12 * ry + 1)
    return out


@pytest.mark.parametrize("cls", F.CLASSES)
def test_income_outcomes_probe_equals_the_oracle(oracle, cls, monkeypatch):
    monkeypatch.delenv("MCR_INCOME_FANOUT_MIN_WAVES", raising=False)
    lib = N.load_library()
    plans, runs = class_runs(oracle, cls)
    assert plans, cls
    for k, (scn, (idx, opts, _)) in enumerate(plans):
        ctx = scn.context("income outcomes probe")
        for o, run in zip(opts, runs[5 * k: 5 * k + 5]):
            assert F.money_scale(run) < F.SCALE_LIMIT, (o, ctx)
        want_fin, want_ruin, scale = oracle_rows(runs, k)
        assert want_fin.shape == want_ruin.shape == scale.shape == (5, scn.n)
        own = scn.cfgd["other_income_streams"][idx]
        money = (scn.cfgd["initial_balance"], scn.cfgd["monthly_contribution"], scn.cfgd["monthly_expenses"])
        records = [money + tuple(o.get(f, own[f]) for f in STREAM_FIELDS) for o in opts]
        counts, fin_t, ruin_t = E.probe_income_outcomes(scn.params(), scn.seed, scn.stream, scn.begin, scn.n, scn.wm, idx, records)
        launches = lib.mcr_probe_income_last_fanout_launches()
        ry = int(scn.cfgd["retirement_years"])
        months = E.ruin_month_counts(ruin_t, scn.n, ry).cpu().numpy()
        fin, ruin = fin_t.cpu().numpy()[:, :scn.n], ruin_t.cpu().numpy()[:, :scn.n]
        assert np.array_equal(np.isnan(fin), np.isnan(want_fin)) and np.array_equal(np.isnan(ruin), np.isnan(want_ruin)), ctx
        assert np.array_equal(np.isnan(ruin), ~np.isnan(fin)), ctx
        np.testing.assert_allclose(ruin, want_ruin, rtol=0, atol=0, equal_nan=True, err_msg=ctx)
        ok = ~np.isnan(want_fin)
        err = np.abs(fin[ok] - want_fin[ok])
        print(f"{cls} plan {k}: max final-balance error {float(err.max()) if err.size else 0.0:.3e}")
        assert np.all(err <= ABS + REL * np.maximum(np.abs(want_fin[ok]), scale[ok])), (ctx, float(err.max()))
        assert months.tolist() == month_counts(want_ruin, ry).tolist(), ctx
        assert counts.cpu().numpy().tolist() == [[int(c), scn.n] for c in ok.sum(axis=1)], ctx
        if cls == "generic":     # 17 or more paying streams, or the exact month: one launch per option
            assert launches == 0, ctx
        else:
            assert launches >= 1, ctx


def test_the_oracles_outcomes_are_mixed(oracle):
    """The comparison above is not vacuous (the reference alone; with the suite's seed: 128 465 path-options of which 73 581
    fail, in 467 distinct ruin months, month 0 included; 256 of the 305 option rows hold both outcomes)."""
    paths = failed = rows = mixed = 0
    months = set()
    for cls in F.CLASSES:
        plans, runs = class_runs(oracle, cls)
        for k in range(len(plans)):
            _, ruin, _ = oracle_rows(runs, k)
            for y in ruin:
                bad = ~np.isnan(y)
                paths += y.size
                failed += int(bad.sum())
                rows += 1
                mixed += bool(bad.any() and not bad.all())
                months.update(np.rint(12.0 * y[bad]).astype(np.int64).tolist())
    assert paths > 0 and 4 * failed >= paths and 4 * (paths - failed) >= paths, (failed, paths)
    assert len(months) >= 100 and 0 in months, len(months)
    assert 2 * mixed >= rows, (mixed, rows)
