"""Every count-only route of the path kernel against the CPU oracle, on the stratified random plans of tests/count_fuzz.py.

The other tests of these routes compare them with one another (fan-out == plain small launch == unsplit kernel == forced lower
mask) on a dozen config.json-derived parameter blocks; an error the MODE 0 instantiations share passes all of them.  Here each
route's integers are compared with the ORACLE's, class by class (count_fuzz.CLASSES: one per compiled tax / annual / generic
variant), on plans calibrated to mixed outcomes whose every path stays below the 2^33 money scale — where this project demands
identical flags, so every comparison is exact.  The one tolerance is the in-kernel histogram's, that of
test_gpu_inkernel_hist.test_bins_vs_oracle_1e5: a path within 1e-8 (relative) of an edge may sit in the neighbouring bin.

Which kernel a launch runs is decided by its size and the environment knobs of tests/test_gpu_growth_forms.py; where a knob is
an error unless the launch took the intended route (a forced form on the split kernel, a segment order on a launch that does
not slice), that error is the proof of the route."""

from __future__ import annotations

import os
from contextlib import contextmanager

import numpy as np
import pytest

import count_fuzz as F
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.stress import assumption_records

pytestmark = pytest.mark.gpu

KNOBS = ("MCR_K1_GROWTH_FORM", "MCR_K1_MONTH_FORM", "MCR_K1_SPLIT_MAX_WAVES", "MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS",
         "MCR_K1_SEGMENT_POLLS", "MCR_K1_SEGMENT_ORDER", "MCR_K1_LDS_LOCK_SLOTS", "MCR_EXPENSE_FANOUT_MIN_WAVES",
         "MCR_CONTRIBUTION_FANOUT_MIN_WAVES", "MCR_SCENARIO_FANOUT_MIN_WAVES", "MCR_ASSUMPTION_FANOUT_MIN_WAVES")
EDGES = np.geomspace(1.0, 1e13, 65)
SPLIT = {"MCR_K1_SEGMENTS": "0"}                                    # the default small launch: the producer / consumer kernel
PLAIN = {"MCR_K1_SPLIT_MAX_WAVES": "0", "MCR_K1_SEGMENTS": "0"}     # the unsplit whole-path kernel, whatever the size
LOWER = {3: (1, 0), 1: (0,), 0: ()}                                 # the growth masks below a launch's own
INTEGERS = ("counters", "ruin_year_bins", "wr_obs_counts")
#: lock columns the producer / consumer form holds beside its doubled stage (plan_path_kernel_lds: 40 KB keep four workgroups
#: resident; 10 240 B of tables + 2 x 12 288 B of stage + the block's counters leave two columns of 2 KB); a plan with more
#: paying frozen streams takes the unsplit kernel at any size
SPLIT_LOCK_SLOTS = 2


@contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _count_only(scn, env, n=None):
    with _env(env):
        return E.run_batch_host(scn.params(), scn.seed, scn.stream, scn.begin, scn.n if n is None else n, scn.wm,
                                want_summary=False, want_trajectories=False, hist_edges=EDGES)


def _same_integers(scn, got, ora, route, env=None):
    for key in INTEGERS:
        assert got[key].astype(np.int64).tolist() == ora[key].astype(np.int64).tolist(), (key, scn.context(route, env))


def _same_histogram(scn, got, ora, route, env=None):
    cohort = ora["final_balance"][ora["success"].astype(bool)]
    exp = np.histogram(cohort, bins=EDGES)[0].astype(np.int64)
    bins = got["hist_bins"].astype(np.int64)
    if not np.array_equal(bins, exp):   # only paths within 1e-8 (relative) of an edge may have moved
        near = sum(int(np.any(np.abs(EDGES - x) <= 1e-8 * np.maximum(1.0, np.abs(EDGES)))) for x in cohort)
        assert np.abs(bins - exp).sum() <= 2 * near, (int(np.abs(bins - exp).sum()), near, scn.context(route, env))
    assert bins.sum() == np.count_nonzero((cohort >= EDGES[0]) & (cohort <= EDGES[-1])), scn.context(route, env)


def _count_only_equals_the_oracle(scn, ora, route, env):
    got = _count_only(scn, env)
    _same_integers(scn, got, ora, route, env)
    _same_histogram(scn, got, ora, route, env)


def _raises(scn, knob, value, env):
    env = dict(env, **{knob: str(value)})
    with pytest.raises(RuntimeError, match=knob):
        _count_only(scn, env)
        pytest.fail("the launch has variants, so it is not the kernel this route is about: " + scn.context("forced form", env))


@pytest.mark.parametrize("cls", F.CLASSES)
def test_whole_path_routes_equal_the_oracle(oracle, cls):
    """The producer / consumer kernel, the unsplit kernel at its own forms and at every lower one, the summary-only kernel
    (MODE 1) and the yearly-bins kernel (MODE 3)."""
    forms = {m: 0 for m in (0, 1, 3)}
    for scn in F.scenarios(oracle, cls):
        ora = F.oracle_run(oracle, scn, trajectories=True)
        assert F.money_scale(ora) < F.SCALE_LIMIT, scn.context()
        p = scn.params()
        with _env({}):
            gf, mf = E.growth_form(p, scn.wm), E.month_form(p, scn.wm)
        forms[gf] += 1
        # --- split: the default small launch.  A forced form is an error on it: the split kernel has no variants
        _count_only_equals_the_oracle(scn, ora, "split", SPLIT)
        if cls != "generic" and scn.frozen_streams() <= SPLIT_LOCK_SLOTS:
            if gf:
                _raises(scn, "MCR_K1_GROWTH_FORM", gf, SPLIT)
            if mf:
                _raises(scn, "MCR_K1_MONTH_FORM", mf, SPLIT)
        # --- unsplit: its own forms, each lower growth mask, the general month.  (The annual-gains and the generic kernels
        # have no variants: one launch.)  Forcing the launch's OWN non-zero form succeeds on a kernel with variants only.
        _count_only_equals_the_oracle(scn, ora, "unsplit", PLAIN)
        if cls not in ("annual", "generic"):
            for m in ((gf,) if gf else ()) + LOWER[gf]:
                _count_only_equals_the_oracle(scn, ora, "unsplit, growth form forced", dict(PLAIN, MCR_K1_GROWTH_FORM=str(m)))
            for m in ((1, 0) if mf else ()):
                _count_only_equals_the_oracle(scn, ora, "unsplit, month form forced", dict(PLAIN, MCR_K1_MONTH_FORM=str(m)))
        else:
            if gf:
                _raises(scn, "MCR_K1_GROWTH_FORM", gf, PLAIN)
        # --- summary-only (MODE 1)
        with _env({}):
            got = E.run_batch_host(p, scn.seed, scn.stream, scn.begin, scn.n, scn.wm, want_trajectories=False)
        _same_integers(scn, got, ora, "summary-only")
        assert np.array_equal(got["success"], ora["success"]), scn.context("summary-only: success")
        assert np.array_equal(got["years_to_ruin"], ora["years_to_ruin"], equal_nan=True), scn.context("summary-only: years_to_ruin")
        # --- year bins (MODE 3) on the default edges
        with _env({}):
            got = E.run_year_bins_host(p, scn.seed, scn.stream, scn.begin, scn.n, scn.wm)
        _same_integers(scn, got, ora, "year bins")
        assert int(got["final_success_bins"].sum()) == int(ora["counters"][0]), scn.context("year bins: final_success_bins")
        rows = got["trajectory_bins"].sum(axis=1).astype(np.int64)
        assert rows.shape == (ora["trajectory"].shape[0],) and np.all(rows == scn.n), (rows.tolist(), scn.context("year bins: trajectory_bins"))
    print(f"{cls}: growth forms of the plans {forms}")


def _moved_rho(rho):
    return rho + 0.3 if rho + 0.3 <= 1.0 else rho - 0.3


@pytest.mark.parametrize("cls", F.CLASSES)
def test_probes_and_fanouts_equal_the_oracle(oracle, cls):
    """The shared-prefix month probes and the expense, contribution, scenario, assumption and grid fan-outs: record k's success
    count is the oracle's for a `Config` with the record's fields replaced."""
    plans = F.scenarios(oracle, cls)
    launches = N.load_library().mcr_probe_assumptions_last_fanout_launches
    todo = []
    for scn in plans:
        c = scn.cfgd
        scn.months = [max(0, scn.wm - 12), scn.wm, scn.wm + 1]
        scn.spend, scn.save = c["monthly_expenses"] * 1.25, c["monthly_contribution"] * 0.5
        scn.market = {"inv1_returns_mean": c["inv1_returns_mean"] - 0.02, "equity_inflation_correlation": _moved_rho(c["equity_inflation_correlation"])}
        todo += [((scn,), dict(wm=m)) for m in scn.months]
        todo += [((scn,), over) for over in (dict(monthly_expenses=scn.spend), dict(monthly_contribution=scn.save),
                                             dict(monthly_contribution=scn.save, monthly_expenses=scn.spend), scn.market,
                                             dict(wm=scn.wm + 1, monthly_expenses=scn.spend))]
    F.oracle_runs(oracle, todo)         # (on host threads; every run is cached and shared)

    def successes(scn, **over):
        return int(F.oracle_run(oracle, scn, **over)["counters"][0])

    for scn in plans:
        c, p, at = scn.cfgd, scn.params(), (scn.seed, scn.stream, scn.begin, scn.n)
        own = successes(scn)
        full = lambda counts: [[int(x), scn.n] for x in counts]     # noqa: E731
        with _env({}):
            got = E.probe_months(p, *at, scn.months).cpu().numpy().tolist()
            assert got == full(successes(scn, wm=m) for m in scn.months), scn.context(f"probe_months {scn.months}")
            got = E.probe_expenses(p, *at, scn.wm, [c["monthly_expenses"], c["monthly_expenses"], scn.spend]).cpu().numpy().tolist()
            assert got == full([own, own, successes(scn, monthly_expenses=scn.spend)]), scn.context("probe_expenses")
            got = E.probe_contributions(p, *at, scn.wm, [c["monthly_contribution"], c["monthly_contribution"], scn.save]).cpu().numpy().tolist()
            assert got == full([own, own, successes(scn, monthly_contribution=scn.save)]), scn.context("probe_contributions")
            triple = (c["initial_balance"], c["monthly_contribution"], c["monthly_expenses"])
            got = E.probe_scenarios(p, *at, scn.wm, [triple, triple, (c["initial_balance"], scn.save, scn.spend)]).cpu().numpy().tolist()
            assert got == full([own, own, successes(scn, monthly_contribution=scn.save, monthly_expenses=scn.spend)]), scn.context("probe_scenarios")
            got = E.probe_assumptions(p, *at, scn.wm, assumption_records(scn.config(), [{}, {}, scn.market])).cpu().numpy().tolist()
            n_launches = launches()
            assert got == full([own, own, successes(scn, **scn.market)]), scn.context(f"probe_assumptions {scn.market}")
            assert (n_launches == 0) if cls == "generic" else (n_launches >= 1), (n_launches, scn.context("probe_assumptions: the route"))
            levels = [c["monthly_expenses"], scn.spend]
            got = E.probe_grid(p, *at, [scn.wm, scn.wm + 1], [levels, levels]).cpu().numpy().tolist()
            want = [full([successes(scn, wm=m), successes(scn, wm=m, monthly_expenses=scn.spend)]) for m in (scn.wm, scn.wm + 1)]
            assert got == want, scn.context(f"probe_grid months {[scn.wm, scn.wm + 1]} levels {levels}")


@pytest.mark.parametrize("cls", F.SLICED_CLASSES)
def test_time_sliced_launches_equal_the_oracle(oracle, cls):
    """The smallest launch that slices (one path block more than the resident slots, 6 workgroups per CU), two segments, in
    both orders: with the order given, a launch that does not slice is an error.  The oracle runs without trajectories on host
    threads; the money scale is the plan's, from a count_fuzz.SAMPLE-path trajectory run and every path's start and final
    balance."""
    import torch

    n = torch.cuda.get_device_properties(0).multi_processor_count * 6 * 256 + 1
    sliced = {"MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENTS": "2", "MCR_K1_SEGMENT_ORDER": "0,1"}
    swapped = dict(sliced, MCR_K1_SEGMENT_ORDER="1,0", MCR_K1_SEGMENT_POLLS="1")
    for scn in (F.sliced_scenario(oracle, cls, n),):
        assert scn.n == n and scn.wm <= 25 and 4 <= scn.cfgd["retirement_years"] <= 8, scn.context()
        sample = F.oracle_run(oracle, scn, n=F.SAMPLE, trajectories=True)
        ora = F.oracle_run_threaded(oracle, scn)
        scale = max(F.money_scale(sample), float(np.abs(ora["start_balance"]).max()), float(np.abs(ora["final_balance"]).max()))
        assert scale < F.SCALE_LIMIT, (scale, scn.context())
        assert int(ora["counters"][1]) == n and 0.05 * n <= int(ora["counters"][0]) <= 0.95 * n, (ora["counters"].tolist(), scn.context())
        for env in (sliced, swapped):
            _same_integers(scn, _count_only(scn, env), ora, "time-sliced", env)
        print(f"{cls}: {n} paths, wm {scn.wm}, {scn.cfgd['retirement_years']} retirement years, {int(ora['counters'][0])} successes, money scale {scale:.3g}")
