"""The history stream's other two schemes (include/mcr.h: MCR_HISTORY_STATIONARY, MCR_HISTORY_COHORTS; history_seek in
csrc/mcr_device.h) on the GPU against their CPU restatement (tests/history_scheme_fuzz.py) and the CPU oracle.

Built like tests/test_gpu_history_stream.py, whose comparison functions and tolerances these are: the restatement picks the
rows with NumPy / Python integers and a Philox of its own, the unchanged oracle runs them through `injected_shocks`, and the
route is also held bit for bit to the engine's injected route fed the same rows."""

from __future__ import annotations

import math
import os

import numpy as np
import pytest

import count_fuzz as F
import history_fuzz as HF
import history_scheme_fuzz as SF
from conftest import REPO
from monte_carlo_retirement_amd import Config, MarketHistory, load_config_from_json, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from test_gpu_count_routes_vs_oracle import EDGES, _env
from test_gpu_numpy_stream_vs_oracle import PER_PATH, same_count_only, same_full_output, same_summary, same_year_bins

pytestmark = pytest.mark.gpu

BLOCK = 12
INTEGERS = ("counters", "ruin_year_bins", "wr_obs_counts")
SCHEMES = (SF.STATIONARY, SF.COHORTS)
PATHS = 10_000


def _rng(scn, scheme, table=None, block=BLOCK):
    return N.history_rng(scn.seed, HF.synthetic_record() if table is None else table, block, scheme)


def _usable(oracle, scn, scheme):
    """The oracle's run of the plan under `scheme`, or None when one of its paths reaches the 2^33 money scale."""
    ora = SF.oracle_run_scheme(oracle, scn, HF.synthetic_record(), BLOCK, scheme)
    return ora if F.money_scale(ora) < F.SCALE_LIMIT else None


def _same_bits(a, b, what, keys=PER_PATH + INTEGERS):
    for key in keys:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (key, what)
        assert a[key].tobytes() == b[key].tobytes(), (key, what)


def _config(**over):
    cfg = Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json")))
    return cfg.model_copy(update={"num_simulations_main": PATHS, "num_simulations_search": PATHS, "seed": 20261019, **over}, deep=True)


def _write_csv(path, months=600, seed=5):
    rng = np.random.default_rng(seed)
    eq, inf, prem = (np.expm1(m + s * rng.standard_normal(months)) for m, s in ((0.006, 0.04), (0.003, 0.004), (0.002, 0.01)))
    with open(path, "w") as fh:
        fh.write("equity,inflation,premium\n")
        for t in range(months):
            fh.write(f"{float(eq[t])!r},{float(inf[t])!r},{float(prem[t])!r}\n")


# ---- 0. the command line ----------------------------------------------------------------------------------------------------------
# (first in the file: a child process's device memory is returned some time after it has ended, and the tests of the next file
#  measure free device memory)
def test_cohort_replay_on_the_command_line(tmp_path):
    """`examples/run_scenario.py --history FILE.csv --history-scheme cohorts --cohorts` prints `historical_cohorts(...)
    .to_document()` with the `market` key (the command line is what this test is about: one child process)."""
    import json
    import subprocess
    import sys

    from monte_carlo_retirement_amd.history import market_document
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    path = tmp_path / "record.csv"
    _write_csv(path)
    h = MarketHistory.from_csv(str(path), inv2=None, premium="premium", scheme="cohorts", first_month="1926-01")
    cfg = Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json")))
    want = RetirementMonteCarloSimulator(cfg, main_seed_override=3, rng="history", market_history=h).historical_cohorts(233).to_document()
    want = dict(want, market=market_document(h, False))
    assert want["market"]["scheme"] == "cohorts" and want["market"]["first_month"] == "1926-01" and want["cohorts"] == 600
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--history", str(path), "--history-scheme", "cohorts", "--history-first-month", "1926-01",
           "--working-months", "233", "--seed", "3", "--cohorts"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == json.loads(json.dumps(want))


# ---- 1. the rows ----------------------------------------------------------------------------------------------------------------
BEGINS = (0, 2 ** 32 - 3, 2 ** 40 + 5)          # (with 63 and 65 paths: begins that are no multiple of H, and the 64-bit modulus)
KEYS = ((0, 12345), (1, 2 ** 40 + 987654321))   # (stream, seed)
MAX_PATHS, MAX_MONTHS = 257, 833


@pytest.mark.parametrize("H", (1, 2, 13, 600, 2048))
def test_rows_equal_the_cpu_restatement(H):
    """mcr_draw_shocks_host_rng = table[rows], byte for byte.  A path's rows are a function of the path and the row alone, so
    one restatement of 257 paths x 833 rows per (B, begin, key) serves every smaller draw as its corner."""
    table = np.random.default_rng(H).standard_normal((H, 3))
    draws = 0
    for B in sorted({1, 5, 12, H, 3 * H + 1, 2 ** 31 - 1}):
        for begin in BEGINS:
            for stream, seed in KEYS:
                want = table[SF.stationary_rows(seed, stream, begin, MAX_PATHS, MAX_MONTHS, H, B)]
                for n_months in sorted({min(m, MAX_MONTHS) for m in (1, 2, 3, 4 * B, 4 * B + 1, MAX_MONTHS)}):
                    for n_paths in (1, 63, 65, MAX_PATHS):
                        got = E.draw_shocks_host(N.history_rng(seed, table, B, SF.STATIONARY), stream, begin, n_paths, n_months, 0.7)
                        assert got.tobytes() == np.ascontiguousarray(want[:n_paths, :n_months]).tobytes(), ("stationary", H, B, n_months, n_paths, begin, stream, seed)
                        draws += 1
    for begin in BEGINS:
        want = table[SF.cohort_rows(begin, MAX_PATHS, MAX_MONTHS, H)]
        for stream, seed in KEYS:
            for n_months in (1, 2, 3, 48, 49, MAX_MONTHS):
                for n_paths in (1, 63, 65, MAX_PATHS):
                    got = E.draw_shocks_host(N.history_rng(seed, table, BLOCK, SF.COHORTS), stream, begin, n_paths, n_months, 0.7)
                    assert got.tobytes() == np.ascontiguousarray(want[:n_paths, :n_months]).tobytes(), ("cohorts", H, n_months, n_paths, begin, stream, seed)
                    draws += 1
    print(f"H = {H}: {draws} draws equal")


# ---- 2.-3. every whole-path kernel of the stream against the oracle, on the plans of count_fuzz ---------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_the_plans_can_go_wrong(oracle, scheme):
    """At most 3 of the 68 plans are left out for their money scale under the scheme, and at least 60 have mixed outcomes."""
    left_out, mixed, total = [], 0, 0
    for cls in F.CLASSES:
        for scn in F.scenarios(oracle, cls):
            total += 1
            ora = SF.oracle_run_scheme(oracle, scn, HF.synthetic_record(), BLOCK, scheme)
            if F.money_scale(ora) >= F.SCALE_LIMIT:
                left_out.append((cls, scn.index))
            elif F.MIXED[0] <= F.failure_share(ora) <= F.MIXED[1]:
                mixed += 1
    print(f"{SF.NAMES[scheme]} on the count_fuzz plans: {total} plans, {len(left_out)} left out for their money scale {left_out}, {mixed} mixed")
    assert total == 68 and len(left_out) <= 3 and mixed >= 60, (total, left_out, mixed)


@pytest.mark.parametrize("cls", F.CLASSES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_full_output_equals_the_oracle_and_the_injected_route(oracle, scheme, cls):
    """MODE 2: flags, ruin bins, counters and observation counts identical to the oracle's on the gathered rows, every per-path
    and trajectory element within the path tolerance; and every array bit-identical to the injected route fed those rows."""
    table = HF.synthetic_record()
    for scn in F.scenarios(oracle, cls):
        ora = _usable(oracle, scn, scheme)
        if ora is None:
            continue
        p = scn.params()
        with _env({}):
            full = E.run_batch_host(p, _rng(scn, scheme), scn.stream, scn.begin, scn.n, scn.wm)
            inj = E.run_batch_host(p, 0, scn.stream, 0, scn.n, scn.wm, injected_shocks=SF.gathered(oracle, scn, table, BLOCK, scheme))
        same_full_output(scn, full, ora, f"{SF.NAMES[scheme]}, full output")
        _same_bits(full, inj, scn.context(f"{SF.NAMES[scheme]} vs injected rows"))


@pytest.mark.parametrize("cls", F.CLASSES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_the_other_modes_equal_the_oracle(oracle, scheme, cls):
    """Count-only with the in-kernel histogram (MODE 0), summary-only (MODE 1) and the yearly bins (MODE 3: the device entry
    point through YearBinsBatch, and the host one)."""
    name = SF.NAMES[scheme]
    for scn in F.scenarios(oracle, cls):
        ora = _usable(oracle, scn, scheme)
        if ora is None:
            continue
        p, at = scn.params(), (_rng(scn, scheme), scn.stream, scn.begin, scn.n)
        with _env({}):
            same_count_only(scn, E.run_batch_host(p, *at, scn.wm, want_summary=False, want_trajectories=False, hist_edges=EDGES), ora,
                            f"{name}, count-only")
            same_summary(scn, E.run_batch_host(p, *at, scn.wm, want_trajectories=False), ora, f"{name}, summary-only")
            yb = E.YearBinsBatch(p, scn.wm)
            yb.launch(*at)
            same_year_bins(scn, yb.host(), ora, f"{name}, year bins")
            same_year_bins(scn, E.run_year_bins_host(p, *at, scn.wm), ora, f"{name}, year bins (host buffers)")


# ---- 4. shapes where the cursor can go wrong ------------------------------------------------------------------------------------
def _frozen_plan(oracle, frozen):
    for cls in ("equal_rates", "unequal_rates", "mask1", "mask2", "mask0", "annual"):
        for scn in F.scenarios(oracle, cls):
            if scn.frozen_streams() == frozen:
                return scn
    raise AssertionError(f"no lean plan with {frozen} frozen streams")


def _against_oracle_and_injected(oracle, scn, scheme, table, block, wm=None):
    wm = scn.wm if wm is None else wm
    ora = SF.oracle_run_scheme(oracle, scn, table, block, scheme, wm=wm)
    assert F.money_scale(ora) < F.SCALE_LIMIT, scn.context("money scale")
    p = scn.params()
    with _env({}):
        full = E.run_batch_host(p, _rng(scn, scheme, table, block), scn.stream, scn.begin, scn.n, wm)
        inj = E.run_batch_host(p, 0, scn.stream, 0, scn.n, wm, injected_shocks=SF.gathered(oracle, scn, table, block, scheme, wm=wm))
        count = E.run_batch_host(p, _rng(scn, scheme, table, block), scn.stream, scn.begin, scn.n, wm, want_summary=False, want_trajectories=False,
                                 hist_edges=EDGES)
    route = f"{SF.NAMES[scheme]}, H = {len(table)}, B = {block}, wm = {wm}"
    moved = scn if wm == scn.wm else F.Scenario(scn.cls, scn.index, scn.cfgd, wm, scn.seed, scn.stream, scn.begin, scn.n)
    same_full_output(moved, full, ora, route)       # (the comparison functions name the plan's own months in their messages only)
    same_count_only(moved, count, ora, route + ", count-only")
    _same_bits(full, inj, scn.context(route + " vs injected rows"))


def test_stationary_block_lengths_at_both_ends_and_no_working_months(oracle):
    """B = 1 (every month a restart), B = 2^31 - 1 (practically none after row 0), and launches without accumulation months."""
    table = HF.synthetic_record()
    scn = F.scenarios(oracle, "unequal_rates")[1]          # (index % 4 == 1: a volatile equity series; path_begin = 2^40)
    _against_oracle_and_injected(oracle, scn, SF.STATIONARY, table, 1)
    _against_oracle_and_injected(oracle, scn, SF.STATIONARY, table, 2 ** 31 - 1)
    _against_oracle_and_injected(oracle, scn, SF.STATIONARY, table, BLOCK, wm=0)
    _against_oracle_and_injected(oracle, F.scenarios(oracle, "annual")[0], SF.STATIONARY, table, 5, wm=0)


def test_stationary_on_the_longest_record_beside_lock_columns_and_extended_streams(oracle):
    """H = 2048 (48 KB of factors in LDS): with two frozen income streams, whose lock columns share the workgroup's LDS with
    the table, and on a generic plan of 17 or more paying streams (the extended-stream kernels)."""
    table = HF.synthetic_record(2048)
    _against_oracle_and_injected(oracle, _frozen_plan(oracle, 2), SF.STATIONARY, table, BLOCK)
    many = F.scenarios(oracle, "generic")[0]
    assert sum(1 for s in many.cfgd["other_income_streams"] if s["monthly_amount_today"] != 0.0) >= 17
    _against_oracle_and_injected(oracle, many, SF.STATIONARY, table, BLOCK)


def test_cohorts_on_a_record_shorter_than_any_horizon_and_on_the_longest(oracle):
    """H = 13: every cohort wraps around the record many times.  H = 2048: the longest table."""
    scn = F.scenarios(oracle, "unequal_rates")[1]
    assert int(oracle.query_sizes(scn.params(), scn.wm).shock_rows) > 10 * 13
    _against_oracle_and_injected(oracle, scn, SF.COHORTS, HF.synthetic_record(13), BLOCK)
    _against_oracle_and_injected(oracle, scn, SF.COHORTS, HF.synthetic_record(2048), BLOCK)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_a_path_range_cut_in_pieces_is_the_same_run(oracle, scheme):
    scn = F.scenarios(oracle, "unequal_rates")[1]
    p = scn.params()
    with _env({}):
        whole = E.run_batch_host(p, _rng(scn, scheme), scn.stream, scn.begin, 1000, scn.wm)
        parts = [E.run_batch_host(p, _rng(scn, scheme), scn.stream, scn.begin + b, m, scn.wm) for b, m in ((0, 333), (333, 1), (334, 666))]
    for key in PER_PATH:
        assert np.concatenate([q[key] for q in parts], axis=-1).tobytes() == whole[key].tobytes(), key
    for key in INTEGERS:
        assert sum(q[key].astype(np.int64) for q in parts).tolist() == whole[key].astype(np.int64).tolist(), key
    assert int(whole["counters"][1]) == 1000


def test_cohorts_repeat_after_one_record(oracle):
    """Paths i and i + H are the same path: of 2 H paths the second half is the first, byte for byte."""
    scn = F.scenarios(oracle, "unequal_rates")[1]
    H = HF.RECORD_MONTHS
    with _env({}):
        r = E.run_batch_host(scn.params(), _rng(scn, SF.COHORTS), scn.stream, scn.begin, 2 * H, scn.wm)
    for key in PER_PATH:
        assert np.ascontiguousarray(r[key][..., :H]).tobytes() == np.ascontiguousarray(r[key][..., H:]).tobytes(), key
    assert 0 < int(r["counters"][0]) < 2 * H and int(r["counters"][0]) % 2 == 0


# ---- 5. scheme 0 is untouched ---------------------------------------------------------------------------------------------------
def test_an_explicit_block_scheme_is_the_descriptor_it_always_was(oracle):
    scn = F.scenarios(oracle, "unequal_rates")[1]
    p, table = scn.params(), HF.synthetic_record()
    old = N.history_rng(scn.seed, table, BLOCK)
    new = N.history_rng(scn.seed, table, BLOCK, scheme=N.MCR_HISTORY_BLOCK)
    assert old.history_scheme == new.history_scheme == 0 and old.history_reserved == new.history_reserved == 0
    with _env({}):
        a = E.run_batch_host(p, old, scn.stream, scn.begin, scn.n, scn.wm)
        b = E.run_batch_host(p, new, scn.stream, scn.begin, scn.n, scn.wm)
    _same_bits(a, b, scn.context("scheme = 0 given explicitly"))
    same_full_output(scn, b, HF.oracle_run_history(oracle, scn, table, BLOCK), "block scheme, full output")


# ---- 6. through the class -------------------------------------------------------------------------------------------------------
def _plain_successes(sim, cfg, stream, wm, n=PATHS):
    """Successes of a plain count-only launch of `cfg` on the simulator's history descriptor."""
    r = E.run_batch_host(params_from_config(cfg), sim._batch_rng(n), stream, 0, n, wm, want_summary=False, want_trajectories=False)
    assert int(r["counters"][1]) == n
    return int(r["counters"][0])


def test_simulator_on_a_stationary_history(oracle):
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = _config()
    h = MarketHistory(HF.synthetic_record(), block_months=BLOCK, scheme="stationary")
    sim = RetirementMonteCarloSimulator(cfg, rng="history", market_history=h)
    assert sim._batch_rng(PATHS).history_scheme == N.MCR_HISTORY_STATIONARY
    wm = 233
    out = sim.run_monte_carlo_simulations(wm, PATHS)
    assert len(out[0]) == PATHS
    plain = _plain_successes(sim, cfg, N.MCR_STREAM_FINAL, wm)
    assert sim._success_probability(out[0]) == float(np.float64(plain) / np.float64(PATHS) * 100.0) and 0 < plain < PATHS
    # and that count is the oracle's on the restated rows
    rows = int(oracle.query_sizes(params_from_config(cfg), wm).shock_rows)
    shocks = h.z[SF.stationary_rows(sim._engine_seed, N.MCR_STREAM_FINAL, 0, PATHS, rows, h.months, BLOCK)]
    ora = oracle.run_batch(params_from_config(cfg), 0, N.MCR_STREAM_FINAL, 0, PATHS, wm, injected_shocks=shocks, want_trajectories=False)
    assert plain == int(ora["counters"][0])

    first = sim.find_maximum_monthly_expenses(wm, verbose=False)
    again = RetirementMonteCarloSimulator(cfg, rng="history", market_history=h).find_maximum_monthly_expenses(wm, verbose=False)
    assert first[0] == again[0] and first[1] == again[1] and first[0] > 0
    count = _plain_successes(sim, cfg.model_copy(update={"monthly_expenses": first[0]}), N.MCR_STREAM_SEARCH, wm)
    assert first[1] == count / PATHS * 100.0 and first[1] >= cfg.target_probability


def test_historical_cohorts(oracle):
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = _config(monthly_expenses=12_000.0)
    H, wm = HF.RECORD_MONTHS, 233
    h = MarketHistory(HF.synthetic_record(), scheme="cohorts", first_month="1926-01")
    sim = RetirementMonteCarloSimulator(cfg, rng="history", market_history=h)
    sim.use_search_seeds()          # (the replay runs on the final stream whatever the active one)
    replay = sim.historical_cohorts(wm)
    p = params_from_config(cfg)
    direct = E.run_batch_host(p, N.history_rng(sim._engine_seed, h.z, h.block_months, N.MCR_HISTORY_COHORTS), N.MCR_STREAM_FINAL, 0, H, wm,
                              want_trajectories=False)
    assert len(replay) == H and replay.start_row.tolist() == list(range(H))
    assert replay.success.tolist() == direct["success"].astype(bool).tolist()
    assert replay.final_balance.tobytes() == direct["final_balance"].tobytes() and replay.years_to_ruin.tobytes() == direct["years_to_ruin"].tobytes()
    sizes = oracle.query_sizes(p, wm)
    ora = oracle.run_batch(p, 0, N.MCR_STREAM_FINAL, 0, H, wm, injected_shocks=h.z[SF.cohort_rows(0, H, int(sizes.shock_rows), H)], want_trajectories=False)
    assert replay.success.tolist() == np.asarray(ora["success"]).astype(bool).tolist()
    total = int(sizes.total_months)
    assert total == wm + 12 * cfg.retirement_years and replay.total_months == total
    assert replay.wraps.tolist() == [i + total > H for i in range(H)]
    assert replay.wraps.all() and replay.success_probability_complete is None        # 833 months a path, 600 in the record
    assert replay.start_month[0] == "1926-01" and replay.start_month[13] == "1927-02"
    ok = int(replay.success.sum())
    assert 0 < ok < H and replay.success_probability == float(np.float64(ok) / np.float64(H) * 100.0)
    # a record longer than the horizon has complete cohorts: starts 0 .. H - total
    long = RetirementMonteCarloSimulator(cfg, rng="history", market_history=MarketHistory(HF.synthetic_record(2048), scheme="cohorts")).historical_cohorts(wm)
    assert long.wraps.tolist() == [i + total > 2048 for i in range(2048)] and int((~long.wraps).sum()) == 2048 - total + 1
    complete = ~long.wraps
    assert long.success_probability_complete == float(np.float64(int(long.success[complete].sum())) / np.float64(int(complete.sum())) * 100.0)
    assert long.start_month == [None] * 2048 and 0 < int(long.success.sum()) < 2048
    worst = replay.worst(5)
    assert len(worst) == 5 and not replay.success[worst[0]] and replay.years_to_ruin[worst[0]] == np.nanmin(np.where(replay.success, np.nan, replay.years_to_ruin))
    # n paths, n a multiple of H: the batch probability is the replay's
    out = sim.run_monte_carlo_simulations(wm, 2 * H)
    assert sim._success_probability(out[0]) == replay.success_probability


# ---- 7. one statistical check ---------------------------------------------------------------------------------------------------
def test_the_stationary_bootstrap_agrees_with_the_block_bootstrap_on_an_iid_record():
    """A record of 600 standardised i.i.d. normal rows, read around the config's own market: whatever the block rule, a path's
    months are (nearly) independent draws from the record, so the stationary and the fixed-block streams at B = 12 sample the
    same law (blocks of consecutive i.i.d. rows carry no dependence to keep).  Two independent binomial estimates over 10 000
    paths each: the difference has standard error sqrt(p1 q1 / n + p2 q2 / n), and four of those is the bound.  Fixed seeds:
    the outcome is deterministic."""
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = _config()
    z = np.random.default_rng(20261019).standard_normal((600, 3))
    z = (z - z.mean(axis=0)) / z.std(axis=0)
    wm = 200                                      # (config.json succeeds on nearly every path at 233 months, on about a third at 200)
    prob = {}
    for scheme, seed in (("stationary", 11), ("block", 12)):      # (two seeds: independent samples)
        sim = RetirementMonteCarloSimulator(cfg, main_seed_override=seed, rng="history", market_history=MarketHistory(z, BLOCK, scheme=scheme))
        prob[scheme] = sim._success_probability(sim.run_monte_carlo_simulations(wm, PATHS)[0]) / 100.0
    p1, p2 = prob["stationary"], prob["block"]
    se = math.sqrt(p1 * (1.0 - p1) / PATHS + p2 * (1.0 - p2) / PATHS)
    print(f"stationary {100 * p1:.2f} %, fixed blocks {100 * p2:.2f} %, standard error of the difference {100 * se:.3f} points")
    assert 0.05 < p2 < 0.95, p2          # a probability at which the two could differ
    assert abs(p1 - p2) <= 4.0 * se, (p1, p2, se)
