"""The NumPy-stream path kernels (rng="numpy": path_kernel<MODE, 1, ...>) against NumPy itself and the CPU oracle, on the
stratified random plans of tests/count_fuzz.py.

rng="numpy" is the mode whose results equal the reference's for the same seed, and it runs instantiations of its own: output
modes 0-3 x (tax form 0 | 3) x (annual-gains tax off | on), and the generic extended-stream form with the tolerance and with the
exact month.  The recorded fixtures reach a few full-output blocks of them; every other test of this stream compares it with
itself.  Here the reference side is independent of the library: NumPy draws each path's shocks (count_fuzz.numpy_shocks:
SeedSequence -> default_rng -> standard_normal -> the rho mix, as the reference's _draw_shock_path does) and the oracle, pinned
bit for bit to the reference, takes them through `injected_shocks`.  Every plan stays below the 2^33 money scale, where this
project demands identical outcomes: flags and integers are compared exactly, money within the path tolerance of
test_gpu_differential.py, histograms and yearly bins under the existing edge rule.  No tolerance is new.

A flipped flag is a finding.  `_diagnose` then draws the DEVICE's shocks for the plan (draw_shocks_host), injects them into the
oracle and says which side moved: the generator (the oracle on the device's shocks agrees with the kernel) or the path
arithmetic (it agrees with the oracle on NumPy's)."""

from __future__ import annotations

import numpy as np
import pytest

import bin_rule
import count_fuzz as F
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.stress import assumption_records
from test_gpu_count_routes_vs_oracle import EDGES, _env, _moved_rho, _same_histogram, _same_integers
from test_gpu_differential import ABS, REL

pytestmark = pytest.mark.gpu

ALL = F.CLASSES + (F.EXTRA,)
SUMMARY = ("start_balance", "final_balance", "first_year_gross_withdrawal", "first_year_real_gross_withdrawal", "inflation_at_retirement")
PER_PATH = E.SUMMARY_FIELDS + ("success", "trajectory", "real_trajectory", "withdrawal_rate_trajectory")
TABLES = ("trajectory_bins", "real_trajectory_bins", "wr_bins", "final_success_bins")
CUT = {"mask0": 4, "annual": 5, "generic": 4}      # plans with a non-zero child offset AND a non-zero path_begin (count_fuzz.numpy_leg)


def _rng(scn):
    main, off, _ = F.numpy_leg(scn)
    return N.numpy_rng(main, child_offset=off)


def _at(scn):
    """(seed, stream_id, path_begin, n_paths) of the plan's launch on the NumPy stream."""
    return _rng(scn), scn.stream, F.numpy_leg(scn)[2], scn.n


def _ctx(scn, route):
    return scn.context(f"{route}; NumPy stream (main_seed, child_offset, path_begin) = {F.numpy_leg(scn)}")


# ---- the comparisons (tests/test_count_fuzz_cpu.py and tests/test_bin_rule_cpu.py feed them perturbed oracle runs: they can fail) ----
# `ctx(scn, route)`: the text a failure names the launch by.  The default names the plan's NumPy leg; a caller on another stream
# (tests/test_gpu_output_modes_vs_oracle.py: the default Philox stream) passes its own.  What is asserted does not depend on it.
def same_flags(scn, got, ora, route, ctx=_ctx):
    assert np.array_equal(got["success"], ora["success"]), (np.nonzero(got["success"] != ora["success"])[0].tolist(), ctx(scn, route + ": success"))
    assert np.array_equal(got["years_to_ruin"], ora["years_to_ruin"], equal_nan=True), ctx(scn, route + ": years_to_ruin")


def within_path_tolerance(scn, got, ora, keys, route, ctx=_ctx):
    """test_gpu_differential.py's: ABS + REL max(|ref|, the path's own money scale)."""
    scale = np.maximum(1.0, np.abs(ora["trajectory"]).max(axis=0))
    for key in keys:
        assert got[key].shape == ora[key].shape, (key, got[key].shape, ora[key].shape, ctx(scn, route))
        err = np.abs(got[key] - ora[key])
        assert np.all(err <= ABS + REL * np.maximum(np.abs(ora[key]), scale)), (key, float(np.nanmax(err)), ctx(scn, route))


def same_full_output(scn, got, ora, route="full output", ctx=_ctx):
    _same_integers(scn, got, ora, route)
    same_flags(scn, got, ora, route, ctx)
    within_path_tolerance(scn, got, ora, ("trajectory", "real_trajectory") + SUMMARY, route, ctx)
    gw, cw = got["withdrawal_rate_trajectory"], ora["withdrawal_rate_trajectory"]
    assert np.array_equal(np.isnan(gw), np.isnan(cw)), ctx(scn, route + ": withdrawal-rate NaN pattern")
    np.testing.assert_allclose(gw, cw, rtol=1e-8, atol=1e-9, equal_nan=True, err_msg=ctx(scn, route))    # (test_gpu_differential.py's)


def same_summary(scn, got, ora, route="summary-only", ctx=_ctx):
    _same_integers(scn, got, ora, route)
    same_flags(scn, got, ora, route, ctx)
    within_path_tolerance(scn, got, ora, SUMMARY, route, ctx)


def same_count_only(scn, got, ora, route="count-only"):
    _same_integers(scn, got, ora, route)
    _same_histogram(scn, got, ora, route)


def _cells(row, edges):
    return bin_rule.cells(row, edges)


def year_bin_rows(got, ora):
    """(table name, the oracle's rows, the table's edges) of the four yearly tables."""
    ok = ora["success"].astype(bool)
    return [("trajectory_bins", ora["trajectory"], got["edges"]), ("real_trajectory_bins", ora["real_trajectory"], got["edges"]),
            ("wr_bins", ora["withdrawal_rate_trajectory"], got["wr_edges"]), ("final_success_bins", ora["final_balance"][ok][None, :], got["edges"])]


def same_year_bins(scn, got, ora, route="year bins", ctx=_ctx):
    """Every row of the four tables under the rule of tests/bin_rule.py: a row that is not equal may move at most 2 x its entries
    within 1e-8 (relative) of an edge, the edge at 0 apart; every row holds each of its entries once, none below 0."""
    _same_integers(scn, got, ora, route)
    for name, data, edges in year_bin_rows(got, ora):
        table = got[name].astype(np.int64).reshape(data.shape[0], -1)
        for t, row in enumerate(data):
            if name in ("trajectory_bins", "real_trajectory_bins"):
                assert np.count_nonzero(~np.isnan(row)) == scn.n, (name, t, ctx(scn, route))
            _, _, wrong = bin_rule.row_verdict(table[t], row, edges)
            assert wrong is None, (f"{name}[{t}]: {wrong}", ctx(scn, route))


# ---- a. the four whole-path launches ------------------------------------------------------------------------------------------
def _diagnose(oracle, scn, got, ora):
    """Which side moved on a flipped flag: the oracle on the DEVICE's own shocks against the kernel and against NumPy's."""
    rows = int(oracle.query_sizes(scn.params(), scn.wm).shock_rows)
    dev = E.draw_shocks_host(*_at(scn), rows, scn.cfgd["equity_inflation_correlation"])
    ref = F.numpy_shocks(scn)
    on_dev = oracle.run_batch(scn.params(), 0, scn.stream, 0, scn.n, scn.wm, injected_shocks=dev, want_trajectories=False)
    same_ruin = (got["years_to_ruin"] == ora["years_to_ruin"]) | (np.isnan(got["years_to_ruin"]) & np.isnan(ora["years_to_ruin"]))
    flip = np.nonzero((got["success"] != ora["success"]) | ~same_ruin)[0]
    gen = np.nonzero(on_dev["success"] != ora["success"])[0]
    arith = np.nonzero(on_dev["success"] != got["success"])[0]
    return (f"flipped paths {flip.tolist()}; shocks: max |device - NumPy| = {float(np.abs(dev - ref).max()):.3g}, "
            f"{int((dev.view(np.uint64) != ref.view(np.uint64)).sum())} values differ in bits; the oracle on the device's shocks differs from "
            f"the oracle on NumPy's on paths {gen.tolist()} (the GENERATOR moved them) and from the kernel on paths {arith.tolist()} "
            f"(the PATH ARITHMETIC moved them)")


@pytest.mark.parametrize("cls", ALL)
def test_whole_path_kernels_equal_the_oracle(oracle, cls):
    """Full output (MODE 2), summary-only (1), count-only with the in-kernel histogram (0) and yearly bins (3) of every plan."""
    plans = F.numpy_plans(oracle, cls)
    for scn in plans:
        ora = F.oracle_run_numpy(oracle, scn, trajectories=True)
        assert F.money_scale(ora) < F.SCALE_LIMIT, _ctx(scn, "money scale")
        p, at = scn.params(), _at(scn)
        with _env({}):
            full = E.run_batch_host(p, *at, scn.wm)
            if not (np.array_equal(full["success"], ora["success"]) and np.array_equal(full["years_to_ruin"], ora["years_to_ruin"], equal_nan=True)):
                pytest.fail(_diagnose(oracle, scn, full, ora) + " -- " + _ctx(scn, "full output"))
            same_full_output(scn, full, ora)
            same_summary(scn, E.run_batch_host(p, *at, scn.wm, want_trajectories=False), ora)
            same_count_only(scn, E.run_batch_host(p, *at, scn.wm, want_summary=False, want_trajectories=False, hist_edges=EDGES), ora)
            same_year_bins(scn, E.run_year_bins_host(p, *at, scn.wm), ora)
    # a forced growth form is an error on this stream: its kernels have no variants (growth_form_of: has_variants is false)
    scn = plans[0]
    with _env({"MCR_K1_GROWTH_FORM": "1"}), pytest.raises(RuntimeError, match="MCR_K1_GROWTH_FORM"):
        E.run_batch_host(scn.params(), *_at(scn), scn.wm, want_summary=False, want_trajectories=False)


# ---- b. the probes: on this stream each takes the one-launch-per-option route -------------------------------------------------
@pytest.mark.parametrize("cls", ALL)
def test_probes_on_the_numpy_stream_equal_the_oracle(oracle, cls, monkeypatch):
    """Record k's success count is the oracle's for a `Config` with the record's fields replaced, on NumPy's shocks: redrawn for
    another working-month count (shock_rows moves), mixed again for a moved rho, unchanged for a probed income stream."""
    from test_gpu_income_vs_oracle import plan_jobs
    from test_gpu_joint_outcomes import unpack

    monkeypatch.delenv("MCR_INCOME_FANOUT_MIN_WAVES", raising=False)
    lib = N.load_library()

    def run(scn, **over):
        ora = F.oracle_run_numpy(oracle, scn, trajectories=True, **over)
        assert F.money_scale(ora) < F.SCALE_LIMIT, (over, _ctx(scn, "money scale"))
        return ora

    for k, scn in enumerate(F.numpy_plans(oracle, cls)[:3]):
        c, p, at = scn.cfgd, scn.params(), _at(scn)
        successes = lambda **over: int(run(scn, **over)["counters"][0])     # noqa: E731
        full = lambda counts: [[int(x), scn.n] for x in counts]            # noqa: E731
        months = [max(0, scn.wm - 12), scn.wm, scn.wm + 1]
        spend, save = c["monthly_expenses"] * 1.25, c["monthly_contribution"] * 0.5
        market = {"inv1_returns_mean": c["inv1_returns_mean"] - 0.02, "equity_inflation_correlation": _moved_rho(c["equity_inflation_correlation"])}
        own = successes()
        with _env({}):
            got = E.probe_months(p, *at, months).cpu().numpy().tolist()
            assert got == full(successes(wm=m) for m in months), _ctx(scn, f"probe_months {months}")
            got = E.probe_expenses(p, *at, scn.wm, [c["monthly_expenses"], c["monthly_expenses"], spend]).cpu().numpy().tolist()
            assert got == full([own, own, successes(monthly_expenses=spend)]), _ctx(scn, "probe_expenses")
            got = E.probe_contributions(p, *at, scn.wm, [c["monthly_contribution"], c["monthly_contribution"], save]).cpu().numpy().tolist()
            assert got == full([own, own, successes(monthly_contribution=save)]), _ctx(scn, "probe_contributions")
            triple = (c["initial_balance"], c["monthly_contribution"], c["monthly_expenses"])
            triples = [triple, triple, (c["initial_balance"], save, spend)]
            moved = run(scn, monthly_contribution=save, monthly_expenses=spend)
            got = E.probe_scenarios(p, *at, scn.wm, triples).cpu().numpy().tolist()
            assert got == full([own, own, int(moved["counters"][0])]), _ctx(scn, "probe_scenarios")
            got = E.probe_assumptions(p, *at, scn.wm, assumption_records(scn.config(), [{}, {}, market])).cpu().numpy().tolist()
            launches = lib.mcr_probe_assumptions_last_fanout_launches()
            assert got == full([own, own, successes(**market)]), _ctx(scn, f"probe_assumptions {market}")
            assert launches == 0, (launches, _ctx(scn, "probe_assumptions: the route"))
            levels = [c["monthly_expenses"], spend]
            got = E.probe_grid(p, *at, [scn.wm, scn.wm + 1], [levels, levels]).cpu().numpy().tolist()
            want = [full([successes(wm=m), successes(wm=m, monthly_expenses=spend)]) for m in (scn.wm, scn.wm + 1)]
            assert got == want, _ctx(scn, f"probe_grid months {[scn.wm, scn.wm + 1]} levels {levels}")
            jobs = plan_jobs(scn)
            if jobs is not None:
                idx, opts, lists = jobs
                stream = c["other_income_streams"][idx]
                records = [triple + tuple(o.get(f, stream[f]) for f in ("monthly_amount_today", "start_at_age", "duration_years")) for o in opts]
                got = E.probe_income(p, *at, scn.wm, idx, records).cpu().numpy().tolist()
                launches = lib.mcr_probe_income_last_fanout_launches()
                assert got == full(successes(other_income_streams=streams) for streams in lists), (idx, opts, _ctx(scn, "probe_income"))
                assert launches == 0, (launches, _ctx(scn, "probe_income: the route"))
            if k == 0:      # the joint form: each option's per-path bits are the oracle's success column
                counts, _, _, masks = E.probe_scenarios_joint(p, *at, scn.wm, triples)
                flags, tail = unpack(masks, scn.n)
                want = np.stack([run(scn)["success"], run(scn)["success"], moved["success"]]).astype(np.uint8)
                assert np.array_equal(flags, want), _ctx(scn, "probe_scenarios_joint: masks")
                assert not tail.any(), _ctx(scn, "probe_scenarios_joint: tail bits")
                assert counts.cpu().numpy().tolist() == full(want.sum(axis=1)), _ctx(scn, "probe_scenarios_joint: counts")


# ---- c. a path range cut in pieces (test_gpu_many_streams.py leaves this out for the NumPy stream) ----------------------------
def test_a_path_range_cut_in_pieces_is_the_same_run(oracle):
    """The child index of a path is child_offset + path_begin + i whatever the launch it runs in, and explicit `path_seeds`
    from SeedSequence are the seeds the kernel derives: both give the whole launch's per-path outputs bit for bit."""
    for cls, index in CUT.items():
        scn = F.scenarios(oracle, cls)[index]
        _, off, begin = F.numpy_leg(scn)
        assert off > 0 and begin > 0 and scn.n > 256, _ctx(scn, "cut")
        p = scn.params()
        with _env({}):
            whole = E.run_batch_host(p, _rng(scn), scn.stream, begin, scn.n, scn.wm)
            parts = [E.run_batch_host(p, _rng(scn), scn.stream, b, m, scn.wm) for b, m in ((begin, 1), (begin + 1, 255), (begin + 256, scn.n - 256))]
            seeded = E.run_batch_host(p, N.numpy_rng(0), scn.stream, 0, scn.n, scn.wm, path_seeds=F.numpy_path_seeds(scn))
        for key in PER_PATH:
            cut = np.concatenate([q[key] for q in parts], axis=-1)
            assert np.array_equal(cut, whole[key], equal_nan=True), (key, _ctx(scn, "cut in pieces"))
            assert np.array_equal(seeded[key], whole[key], equal_nan=True), (key, _ctx(scn, "explicit path_seeds"))
        for key in ("counters", "ruin_year_bins", "wr_obs_counts"):
            assert sum(q[key].astype(np.int64) for q in parts).tolist() == whole[key].astype(np.int64).tolist() == seeded[key].astype(np.int64).tolist(), key
