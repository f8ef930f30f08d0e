"""The history stream (rng="history"; include/mcr.h: MCR_RNG_HISTORY; path_kernel<MODE, 2, ...>) on the GPU against its CPU
restatement (tests/history_fuzz.py) and the CPU oracle.

The stream is defined by which row of the record a path's month reads; the oracle takes rows through `injected_shocks`.  So
the reference side is independent of the library: `history_rows` picks the rows with NumPy integers and a Philox of its own,
the unchanged oracle runs them.  Flags and integers are compared exactly, money within the path tolerance
tests/test_gpu_numpy_stream_vs_oracle.py uses for the same comparison (its functions are imported), and the route is also held
bit for bit to the engine's injected route fed the same rows: both make the month's growth factors with the same device
function in the same order."""

from __future__ import annotations

import math
import os

import numpy as np
import pytest

import count_fuzz as F
import history_fuzz as HF
from conftest import REPO
from monte_carlo_retirement_amd import Config, MarketHistory, load_config_from_json, params_from_config, with_fitted_market
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from test_gpu_count_routes_vs_oracle import EDGES, _env
from test_gpu_numpy_stream_vs_oracle import PER_PATH, same_count_only, same_full_output, same_summary, same_year_bins

pytestmark = pytest.mark.gpu

BLOCK = 12
INTEGERS = ("counters", "ruin_year_bins", "wr_obs_counts")


def _rng(scn, table=None, block=BLOCK):
    return N.history_rng(scn.seed, HF.synthetic_record() if table is None else table, block)


def _usable(oracle, scn):
    """The oracle's history run of the plan, or None when one of its paths reaches the 2^33 money scale."""
    ora = HF.oracle_run_history(oracle, scn, HF.synthetic_record(), BLOCK)
    return ora if F.money_scale(ora) < F.SCALE_LIMIT else None


def _same_bits(a, b, what):
    for key in PER_PATH + INTEGERS:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (key, what)
        assert a[key].tobytes() == b[key].tobytes(), (key, what)


PATHS = 10_000


def _config(**over):
    cfg = Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json")))
    return cfg.model_copy(update={"num_simulations_main": PATHS, "num_simulations_search": PATHS, "seed": 20261019, **over}, deep=True)


# ---- 0. the response document and the command line -------------------------------------------------------------------------------
# (first in the file: a child process's device memory is returned some time after it has ended, and the tests of the next file
#  measure free device memory)
def test_response_document_and_command_line(tmp_path):
    """`results.run_scenario` adds the `market` key with a history and changes nothing without one; `examples/run_scenario.py
    --history FILE.csv` prints it (the command line is what this test is about: one child process)."""
    import json
    import subprocess
    import sys

    from monte_carlo_retirement_amd import results as R

    rng = np.random.default_rng(5)
    eq, inf, prem = (np.expm1(m + s * rng.standard_normal(120)) for m, s in ((0.006, 0.04), (0.003, 0.004), (0.002, 0.01)))
    path = tmp_path / "record.csv"
    with open(path, "w") as fh:
        fh.write("equity,inflation,premium\n")
        for t in range(120):
            fh.write(f"{float(eq[t])!r},{float(inf[t])!r},{float(prem[t])!r}\n")
    h = MarketHistory.from_csv(str(path), inv2=None, premium="premium", block_months=6)
    cfg = _config(num_simulations_main=2000, num_simulations_search=2000)
    plain = R.run_scenario(cfg, 233, main_seed_override=3)
    doc = R.run_scenario(with_fitted_market(cfg, h), 233, main_seed_override=3, rng="history", market_history=h, market_as_recorded=True)
    assert "market" not in plain and set(doc) == set(plain) | {"market"}
    assert doc["market"] == {"months": 120, "block_months": 6, "as_recorded": True, "fitted": h.fitted_assumptions()}
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--history", str(path), "--history-block", "6", "--history-as-recorded",
           "--working-months", "233", "--paths", "2000", "--seed", "3"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["rng"] == "history" and out["market"] == json.loads(json.dumps(doc["market"])) and out["summary"] == json.loads(json.dumps(doc["summary"]))


# ---- 1. the rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (1, 2, 13, 600, 2048))
def test_rows_equal_the_cpu_restatement(H):
    table = np.random.default_rng(H).standard_normal((H, 3))
    draws = 0
    for B in sorted({1, 5, 12, H, 3 * H + 1}):
        for n_months in sorted({min(m, 833) for m in (1, 4 * B, 4 * B + 1, 833)}):
            for n_paths in (1, 63, 65, 257):
                for begin in (0, 2 ** 32 - 3):
                    for stream, seed in ((0, 12345), (1, 2 ** 40 + 987654321)):
                        got = E.draw_shocks_host(N.history_rng(seed, table, B), stream, begin, n_paths, n_months, 0.7)
                        want = table[HF.history_rows(seed, stream, begin, n_paths, n_months, H, B)]
                        assert got.tobytes() == want.tobytes(), (H, B, n_months, n_paths, begin, stream, seed)
                        draws += 1
    print(f"H = {H}: {draws} draws equal")


# ---- 2.-4. every whole-path kernel of the stream against the oracle, on the plans of count_fuzz ----------------------------------
def test_the_plans_can_go_wrong(oracle):
    """At most 3 of the 68 plans are left out for their money scale on this stream, and at least 60 have mixed outcomes."""
    left_out, mixed, total = [], 0, 0
    for cls in F.CLASSES:
        for scn in F.scenarios(oracle, cls):
            total += 1
            ora = HF.oracle_run_history(oracle, scn, HF.synthetic_record(), BLOCK)
            if F.money_scale(ora) >= F.SCALE_LIMIT:
                left_out.append((cls, scn.index))
            elif F.MIXED[0] <= F.failure_share(ora) <= F.MIXED[1]:
                mixed += 1
    print(f"history stream on the count_fuzz plans: {total} plans, {len(left_out)} left out for their money scale {left_out}, {mixed} mixed")
    assert total == 68 and len(left_out) <= 3 and mixed >= 60, (total, left_out, mixed)


@pytest.mark.parametrize("cls", F.CLASSES)
def test_full_output_equals_the_oracle_and_the_injected_route(oracle, cls):
    """MODE 2: flags, ruin bins, counters and observation counts identical to the oracle's on the gathered rows, every per-path
    and trajectory element within the path tolerance; and every array bit-identical to the injected route fed those rows."""
    table = HF.synthetic_record()
    for scn in F.scenarios(oracle, cls):
        ora = _usable(oracle, scn)
        if ora is None:
            continue
        p = scn.params()
        with _env({}):
            full = E.run_batch_host(p, _rng(scn), scn.stream, scn.begin, scn.n, scn.wm)
            inj = E.run_batch_host(p, 0, scn.stream, 0, scn.n, scn.wm, injected_shocks=HF.gathered(oracle, scn, table, BLOCK))
        same_full_output(scn, full, ora, "history stream, full output")
        _same_bits(full, inj, scn.context("history stream vs injected rows"))


@pytest.mark.parametrize("cls", F.CLASSES)
def test_the_other_modes_equal_the_oracle(oracle, cls):
    """Count-only with the in-kernel histogram (MODE 0), summary-only (MODE 1) and the yearly bins (MODE 3, through
    YearBinsBatch: the device entry point, which takes the table as a device copy)."""
    for scn in F.scenarios(oracle, cls):
        ora = _usable(oracle, scn)
        if ora is None:
            continue
        p, at = scn.params(), (_rng(scn), scn.stream, scn.begin, scn.n)
        with _env({}):
            same_count_only(scn, E.run_batch_host(p, *at, scn.wm, want_summary=False, want_trajectories=False, hist_edges=EDGES), ora,
                            "history stream, count-only")
            same_summary(scn, E.run_batch_host(p, *at, scn.wm, want_trajectories=False), ora, "history stream, summary-only")
            yb = E.YearBinsBatch(p, scn.wm)
            yb.launch(*at)
            same_year_bins(scn, yb.host(), ora, "history stream, year bins")
            same_year_bins(scn, E.run_year_bins_host(p, *at, scn.wm), ora, "history stream, year bins (host buffers)")


# ---- 5. sharding and shapes -----------------------------------------------------------------------------------------------------
def test_a_path_range_cut_in_pieces_is_the_same_run(oracle):
    scn = F.scenarios(oracle, "unequal_rates")[1]
    p = scn.params()
    with _env({}):
        whole = E.run_batch_host(p, _rng(scn), scn.stream, scn.begin, 1000, scn.wm)
        parts = [E.run_batch_host(p, _rng(scn), scn.stream, scn.begin + b, m, scn.wm) for b, m in ((0, 333), (333, 1), (334, 666))]
    for key in PER_PATH:
        assert np.concatenate([q[key] for q in parts], axis=-1).tobytes() == whole[key].tobytes(), key
    for key in INTEGERS:
        assert sum(q[key].astype(np.int64) for q in parts).tolist() == whole[key].astype(np.int64).tolist(), key
    assert int(whole["counters"][1]) == 1000


def _frozen_plan(oracle, frozen):
    for cls in ("equal_rates", "unequal_rates", "mask1", "mask2", "mask0", "annual"):
        for scn in F.scenarios(oracle, cls):
            if scn.frozen_streams() == frozen:
                return scn
    raise AssertionError(f"no lean plan with {frozen} frozen streams")


def _against_oracle_and_injected(oracle, scn, table, block, wm=None):
    wm = scn.wm if wm is None else wm
    ora = HF.oracle_run_history(oracle, scn, table, block, wm=wm)
    assert F.money_scale(ora) < F.SCALE_LIMIT, scn.context("money scale")
    p = scn.params()
    with _env({}):
        full = E.run_batch_host(p, _rng(scn, table, block), scn.stream, scn.begin, scn.n, wm)
        inj = E.run_batch_host(p, 0, scn.stream, 0, scn.n, wm, injected_shocks=HF.gathered(oracle, scn, table, block, wm=wm))
        count = E.run_batch_host(p, _rng(scn, table, block), scn.stream, scn.begin, scn.n, wm, want_summary=False, want_trajectories=False,
                                 hist_edges=EDGES)
    route = f"history stream, H = {len(table)}, B = {block}, wm = {wm}"
    if wm == scn.wm:
        same_full_output(scn, full, ora, route)
        same_count_only(scn, count, ora, route + ", count-only")
    else:       # (the comparison functions name the plan's own months in their messages only)
        moved = F.Scenario(scn.cls, scn.index, scn.cfgd, wm, scn.seed, scn.stream, scn.begin, scn.n)
        same_full_output(moved, full, ora, route)
        same_count_only(moved, count, ora, route + ", count-only")
    _same_bits(full, inj, scn.context(route + " vs injected rows"))


def test_the_longest_record_beside_lock_columns_and_extended_streams(oracle):
    """H = 2048 (48 KB of factors in LDS): with two frozen income streams, whose lock columns share the workgroup's LDS with
    the table, and on a generic plan of 17 or more paying streams (the extended-stream kernels)."""
    table = HF.synthetic_record(2048)
    two = _frozen_plan(oracle, 2)
    _against_oracle_and_injected(oracle, two, table, BLOCK)
    many = F.scenarios(oracle, "generic")[0]
    assert sum(1 for s in many.cfgd["other_income_streams"] if s["monthly_amount_today"] != 0.0) >= 17
    _against_oracle_and_injected(oracle, many, table, BLOCK)


def test_block_lengths_at_both_ends_and_no_working_months(oracle):
    """B = 1 (every month a new start), B beyond the horizon (one start per path), and a launch without accumulation months."""
    table = HF.synthetic_record()
    scn = F.scenarios(oracle, "unequal_rates")[1]          # (index % 4 == 1: a volatile equity series; path_begin = 2^40)
    total = int(oracle.query_sizes(scn.params(), scn.wm).shock_rows)
    _against_oracle_and_injected(oracle, scn, table, 1)
    _against_oracle_and_injected(oracle, scn, table, total + 7)
    _against_oracle_and_injected(oracle, scn, table, 2 ** 31 - 1)
    _against_oracle_and_injected(oracle, scn, table, BLOCK, wm=0)
    _against_oracle_and_injected(oracle, F.scenarios(oracle, "annual")[0], table, 5, wm=0)


# ---- 6. through the class -------------------------------------------------------------------------------------------------------
def _plain_successes(sim, cfg, stream, wm, n=PATHS):
    """Successes of a plain count-only launch of `cfg` on the simulator's history descriptor."""
    r = E.run_batch_host(params_from_config(cfg), sim._batch_rng(n), stream, 0, n, wm, want_summary=False, want_trajectories=False)
    assert int(r["counters"][1]) == n
    return int(r["counters"][0])


def test_simulator_on_a_history(oracle):
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = _config()
    h = MarketHistory(HF.synthetic_record(), block_months=BLOCK)
    sim = RetirementMonteCarloSimulator(cfg, rng="history", market_history=h)
    wm = 233
    out = sim.run_monte_carlo_simulations(wm, PATHS)
    assert len(out) == 7 and len(out[0]) == PATHS
    rows = int(oracle.query_sizes(params_from_config(cfg), wm).shock_rows)
    shocks = h.z[HF.history_rows(sim._engine_seed, N.MCR_STREAM_FINAL, 0, PATHS, rows, h.months, BLOCK)]
    ora = oracle.run_batch(params_from_config(cfg), 0, N.MCR_STREAM_FINAL, 0, PATHS, wm, injected_shocks=shocks, want_trajectories=False)
    assert sim._success_probability(out[0]) == float(np.float64(int(ora["counters"][0])) / np.float64(PATHS) * 100.0)
    assert 0 < int(ora["counters"][0]) < PATHS

    # the working-month search: the count at every month it probed is a plain launch's on the search stream
    months, prob, curve = sim.find_minimum_working_months(verbose=False)
    assert months >= 0 and len(curve) >= 3
    for point in curve:
        plain = _plain_successes(sim, cfg, N.MCR_STREAM_SEARCH, int(point["working_months"]))
        assert point["probability"] == round(plain / PATHS * 100.0, 2), point
    assert prob >= cfg.target_probability

    # three what-if records are three plain launches
    sim.use_final_seeds()
    what_if = [{}, {"monthly_expenses": 12_500.0}, {"initial_balance": 100_000.0, "monthly_contribution": 7_000.0}]
    got = sim.success_probability_by_scenarios(wm, what_if, PATHS)
    want = [_plain_successes(sim, cfg.model_copy(update=w), N.MCR_STREAM_FINAL, wm) / PATHS * 100.0 for w in what_if]
    assert got.tolist() == want
    assert len(set(want)) == 3

    # the spending search terminates, reproduces, and its answer is a plain launch's
    first = sim.find_maximum_monthly_expenses(wm, verbose=False)
    again = RetirementMonteCarloSimulator(cfg, rng="history", market_history=h).find_maximum_monthly_expenses(wm, verbose=False)
    assert first[0] == again[0] and first[1] == again[1] and first[0] > 0
    plain = _plain_successes(sim, cfg.model_copy(update={"monthly_expenses": first[0]}), N.MCR_STREAM_SEARCH, wm)
    assert first[1] == plain / PATHS * 100.0 and first[1] >= cfg.target_probability

    with pytest.raises(ValueError, match="market_history"):
        RetirementMonteCarloSimulator(cfg, rng="history")
    with pytest.raises(ValueError, match="market_history"):
        RetirementMonteCarloSimulator(cfg, rng="philox", market_history=h)


def test_a_lognormal_record_as_recorded_agrees_with_the_engines_own_stream():
    """The one statistical check.  A 2048-month record of independent lognormal draws, resampled month by month (B = 1) around
    its own fitted market, is a sample from (nearly) the model the Philox stream draws from under the same fitted parameters:
    the first two moments of every series and the equity / inflation correlation agree exactly, by construction of the fit.
    The two success probabilities are independent binomial estimates over 10 000 paths each; their difference has standard
    error sqrt(p1 q1 / n + p2 q2 / n), and three of those is the bound.  Fixed seeds: the outcome is deterministic."""
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = _config(monthly_expenses=12_000.0)      # (config.json itself succeeds on nearly every path at 233 months)
    p = params_from_config(cfg)
    rng = np.random.default_rng(20261019)
    z = rng.standard_normal((2048, 3))
    gross = np.exp(np.array([p.inv1_mu_log, p.inf_mu_log, p.prem_mu_log]) / 12.0 + np.array([p.inv1_sigma_log, p.inf_sigma_log, p.prem_sigma_log]) / math.sqrt(12.0) * z)
    h = MarketHistory.from_monthly_returns(gross[:, 0] - 1.0, gross[:, 1] - 1.0, premium=gross[:, 2] - 1.0, block_months=1)
    fit = with_fitted_market(cfg, h)
    wm = 233
    hist = RetirementMonteCarloSimulator(fit, rng="history", market_history=h)
    own = RetirementMonteCarloSimulator(fit, rng="philox")
    ph = hist._success_probability(hist.run_monte_carlo_simulations(wm, PATHS)[0]) / 100.0
    po = own._success_probability(own.run_monte_carlo_simulations(wm, PATHS)[0]) / 100.0
    se = math.sqrt(ph * (1.0 - ph) / PATHS + po * (1.0 - po) / PATHS)
    print(f"history as recorded {100 * ph:.2f} %, Philox under the fitted market {100 * po:.2f} %, standard error of the difference {100 * se:.3f} points")
    assert 0.05 < po < 0.95, po          # a probability at which the two could differ
    assert abs(ph - po) <= 3.0 * se, (ph, po, se)
