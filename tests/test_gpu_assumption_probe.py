"""Assumption probes (`mcr_probe_assumptions_rng`, `engine.probe_assumptions`), the stress table and the break-even assumption
search on the GPU.

The contract: record k's counters equal, bit for bit, those of a count-only launch with the ten fields of the parameter block
(the three scenario levers and the market's seven lognormal parameters) replaced by record k (`engine.probe_months` of the
parameter block of the modified `Config`) — on the assumption fan-out route (Philox, <= 16 streams, tolerance month) and on
the per-record route (NumPy stream, longer stream lists, the exact month, or forced).

Against the CPU oracle (`test_success_counts_equal_the_oracle`): config.json, 233 working months, 256 paths; the oracle counts
251, 256, 210, 2, 40, 203, 253 successes for the seven records, every path's money scale <= 3.4e9 (below the 2^33 at which
test_gpu_differential.py admits knife-edge flips), so the counts must agree exactly."""

from __future__ import annotations

import ctypes as C
import json
import math

import numpy as np
import pytest

from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
from monte_carlo_retirement_amd.stress import assumption_records
from test_gpu_expense_probe import SCENARIOS as EXPENSE_SCENARIOS, _cfg, _stream

pytestmark = pytest.mark.gpu
SEED = 0x5CE_4A10
STRADDLE = 2**32 - 37   # the first wavefront holds paths 2^32 - 37 .. 2^32 + 26 (the producer's general Philox form)

SCENARIOS = {name: EXPENSE_SCENARIOS[name] for name in ("config", "jorge_rho", "no_tax", "annual_tax",
                                                        "streams17", "exact_month")}   # (the last two: per-record route)
#: 8 non-indexed income streams = 8 lock columns per consumer wave: beside PHASE 9's 19 712 B of static LDS, 64 KB hold 11 waves
#: of them (11 x 4 KB + 64 B of counters; a twelfth does not fit), so a launch takes 11 records, 15 go as 8 + 7, 40 as 4 x 10
FROZEN8 = _cfg(other_income_streams=[dict(_stream(i), inflation_indexed=False) for i in range(8)])


def _overrides(cfgd, L):
    """L records as `Config` overrides (a prefix of the list, so from L = 11 on all of these): the config's own values; a
    duplicate; all three volatilities 0; rho = 0, +1, -1 and 0.5 (one launch holds all four from L = 7 on); equity mean -0.4;
    equity volatility 0.9; inflation mean 0.3; initial_balance 0; then a spread in which all ten fields differ."""
    head = [{}, {},
            {"inv1_returns_volatility": 0.0, "inflation_rate_volatility": 0.0, "inv2_premium_over_inflation_volatility": 0.0},
            {"equity_inflation_correlation": 0.0}, {"equity_inflation_correlation": 1.0},
            {"equity_inflation_correlation": -1.0}, {"equity_inflation_correlation": 0.5},
            {"inv1_returns_mean": -0.4}, {"inv1_returns_volatility": 0.9}, {"inflation_rate_mean": 0.3}, {"initial_balance": 0.0}]
    spread = [{"inv1_returns_mean": round(0.01 + 0.006 * k, 4), "inv1_returns_volatility": round(0.03 + 0.011 * k, 4),
               "inflation_rate_mean": round(0.09 - 0.003 * k, 4), "inflation_rate_volatility": round(0.002 * k, 4),
               "inv2_premium_over_inflation_mean": round(-0.01 + 0.002 * k, 4),
               "inv2_premium_over_inflation_volatility": round(0.05 - 0.0015 * k, 4),
               "equity_inflation_correlation": round(-0.9 + 0.06 * k, 4),
               "initial_balance": round(max(float(cfgd["initial_balance"]), 1000.0) * (0.1 + 0.3 * k), 2),
               "monthly_contribution": round(max(float(cfgd["monthly_contribution"]), 100.0) * (2.5 - 0.07 * k), 2),
               "monthly_expenses": round(max(float(cfgd["monthly_expenses"]), 100.0) * (0.4 + 0.05 * k), 2)}
              for k in range(max(0, L - len(head)))]
    return (head + spread)[:L]


_REFERENCE = {}   # (config, seed, stream, path range, month, overrides) -> counters of the plain launch: computed once, shared


def _plain(cfgd, seed, stream, begin, n, wm, over):
    q = params_from_config(Config(**dict(cfgd, **over)))
    if not isinstance(seed, int):   # (a NumPy-stream descriptor: three small cases, not shared)
        return E.probe_months(q, seed, stream, begin, n, [wm]).cpu().numpy()[0].tolist()
    key = (json.dumps(cfgd, sort_keys=True, default=str), seed, stream, begin, n, wm, json.dumps(over, sort_keys=True))
    if key not in _REFERENCE:
        _REFERENCE[key] = E.probe_months(q, seed, stream, begin, n, [wm]).cpu().numpy()[0].tolist()
    return _REFERENCE[key]


def _check(cfgd, seed, wm, n, begin, overrides, stream=0):
    cfg = Config(**cfgd)
    p = params_from_config(cfg)
    got = E.probe_assumptions(p, seed, stream, begin, n, wm, assumption_records(cfg, overrides)).cpu().numpy().tolist()
    want = [_plain(cfgd, seed, stream, begin, n, wm, o) for o in overrides]
    assert got == want, (wm, n, begin, len(overrides))
    return got


def _sweep(cfgd):
    Ls = [1, 2, 8, 15, 16, 40]
    i = 0
    for wm in (0, 1, 13, 233):
        for n in (1, 63, 65, 20_000):
            begin = (0, 12_345)[i % 2]
            L = Ls[i % len(Ls)]
            i += 1
            got = _check(cfgd, SEED, wm, n, begin, _overrides(cfgd, L))
            assert all(c[1] == n for c in got)
            if L >= 2:   # the config's own values: also what the scenario probe counts on the same triple
                own = tuple(float(cfgd[f]) for f in ("initial_balance", "monthly_contribution", "monthly_expenses"))
                p = params_from_config(Config(**cfgd))
                assert E.probe_scenarios(p, SEED, 0, begin, n, wm, [own, own]).cpu().numpy().tolist() == got[:2]


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_counts_equal_plain_launches(name):
    _sweep(SCENARIOS[name])


def test_records_differ_in_their_counts():
    cfgd = SCENARIOS["config"]
    got = _check(cfgd, SEED, 233, 20_000, 0, _overrides(cfgd, 16))
    assert len({c[0] for c in got}) > 1         # the market does reach the consumers: the records do not all count alike
    assert got[7][0] < got[0][0] and got[9][0] < got[0][0]     # equity mean -0.4, inflation mean 0.3


def test_counts_with_fewer_records_per_launch_than_fifteen():
    _sweep(FROZEN8)
    for L in (11, 12, 15, 40):   # one full launch, 6 + 6, 8 + 7, 4 x 10
        _check(FROZEN8, SEED, 120, 2000, 77, _overrides(FROZEN8, L))


def test_counts_with_the_numpy_stream():
    cfgd = SCENARIOS["config"]
    for wm, n, L in ((0, 65, 2), (13, 1000, 8), (233, 5000, 16)):
        rng = N.numpy_rng(1234, child_offset=0)
        _check(cfgd, rng, wm, n, 0, _overrides(cfgd, L), stream=1)


def test_counts_straddling_2_pow_32():
    cfgd = SCENARIOS["config"]
    for n, L in ((65, 8), (20_000, 16)):
        _check(cfgd, SEED, 233, n, STRADDLE, _overrides(cfgd, L))
    _check(SCENARIOS["annual_tax"], SEED, 233, 65, STRADDLE, _overrides(SCENARIOS["annual_tax"], 8))   # (the plain generator)


def test_forced_routes_agree(monkeypatch):
    cfgd = SCENARIOS["config"]
    cfg = Config(**cfgd)
    p = params_from_config(cfg)
    records = assumption_records(cfg, _overrides(cfgd, 15))
    launches = N.load_library().mcr_probe_assumptions_last_fanout_launches
    monkeypatch.setenv("MCR_ASSUMPTION_FANOUT_MIN_WAVES", "0")
    fan = E.probe_assumptions(p, SEED, 0, 0, 20_000, 240, records).cpu().numpy()
    assert launches() == 1                      # the fan-out kernel did run: 15 records, one launch
    monkeypatch.setenv("MCR_ASSUMPTION_FANOUT_MIN_WAVES", str(2**40))
    per = E.probe_assumptions(p, SEED, 0, 0, 20_000, 240, records).cpu().numpy()
    assert launches() == 0                      # ... and here one plain launch per record
    assert fan.tolist() == per.tolist()


def test_the_route_taken_is_the_documented_one(monkeypatch):
    """The calling thread's last probe reports its fan-out launches: ceil(L / records per launch) where the fan-out covers
    the shape, 0 for one record, the NumPy stream, a stream list beyond the inline block and the exact month."""
    monkeypatch.delenv("MCR_ASSUMPTION_FANOUT_MIN_WAVES", raising=False)
    launches = N.load_library().mcr_probe_assumptions_last_fanout_launches

    def run(cfgd, L, seed=SEED):
        cfg = Config(**cfgd)
        E.probe_assumptions(params_from_config(cfg), seed, 0, 0, 130, 13, assumption_records(cfg, _overrides(cfgd, L)))
        return launches()

    cfgd = SCENARIOS["config"]
    assert [run(cfgd, L) for L in (1, 2, 15, 16, 40)] == [0, 1, 1, 2, 3]
    assert [run(FROZEN8, L) for L in (11, 12, 40)] == [1, 2, 4]         # 11 records a launch (FROZEN8 above)
    assert run(SCENARIOS["annual_tax"], 8) == 1 and run(SCENARIOS["no_tax"], 8) == 1
    assert run(SCENARIOS["streams17"], 8) == 0 and run(SCENARIOS["exact_month"], 8) == 0
    assert run(cfgd, 8, seed=N.numpy_rng(1234, child_offset=0)) == 0


ORACLE_RECORDS = [{}, {"inv1_returns_mean": +0.03}, {"inv1_returns_volatility": +0.05}, {"inflation_rate_mean": +0.02},
                  {"inv1_returns_mean": -0.02}, {"inv2_premium_over_inflation_mean": -0.01}, {"equity_inflation_correlation": +0.3}]


def test_success_counts_equal_the_oracle(oracle):
    """Additive shifts of config.json's values; no flips allowed (module docstring)."""
    cfgd = SCENARIOS["config"]
    cfg = Config(**cfgd)
    wm, n = 233, 256
    overrides = [{f: float(cfgd.get(f, 0.0)) + d for f, d in o.items()} for o in ORACLE_RECORDS]
    got = E.probe_assumptions(params_from_config(cfg), SEED, 0, 0, n, wm, assumption_records(cfg, overrides)).cpu().numpy()
    want = [int(oracle.run_batch(params_from_config(Config(**dict(cfgd, **o))), SEED, 0, 0, n, wm)["counters"][0]) for o in overrides]
    print("oracle", want, "gpu", got[:, 0].tolist())
    assert got[:, 0].tolist() == want
    assert got[:, 1].tolist() == [n] * len(overrides)
    assert len(set(want)) > 1


BAD_RECORDS = [("inv1_mu_log", float("nan")), ("inf_mu_log", float("inf")), ("inv1_sigma_log", -0.01), ("prem_sigma_log", -1e-9),
               ("equity_inflation_rho", 1.5), ("equity_inflation_rho", float("nan")), ("initial_balance", -1.0),
               ("monthly_expenses", float("nan")), ("inf_sigma_log", 700.0 * math.sqrt(12.0) / 40.0), ("prem_mu_log", 8400.0)]


def test_invalid_records_leave_counts_untouched(monkeypatch):
    import torch

    cfg = Config(**SCENARIOS["config"])
    p = params_from_config(cfg)
    good = assumption_records(cfg, [{}])[0]
    lib = N.load_library()
    rng = N.McrRng()
    rng.kind, rng.philox_seed = N.MCR_RNG_PHILOX, SEED
    stream = torch.cuda.current_stream(0).cuda_stream
    sentinel = -0x1234_5678
    for field, bad in BAD_RECORDS:
        counts = torch.full((3, 2), sentinel, dtype=torch.int64, device="cuda")
        rec = (N.McrAssumptions * 3)(N.McrAssumptions(*good), N.McrAssumptions(*good), N.McrAssumptions(*good))
        setattr(rec[1], field, bad)
        rc = lib.mcr_probe_assumptions_rng(C.byref(p), C.byref(rng), 0, 0, 1000, 12, rec, 3, C.c_void_p(counts.data_ptr()),
                                           0, C.c_void_p(stream))
        assert rc == N.MCR_ERR_INVALID_ARG and f"records[1].{field}" in N.last_error(), (field, bad, N.last_error())
        torch.cuda.synchronize()
        assert (counts.cpu() == sentinel).all()
    # the block's own ten fields are held to the same rules on every route, although every record replaces them
    for min_waves in ("0", str(2**40)):
        monkeypatch.setenv("MCR_ASSUMPTION_FANOUT_MIN_WAVES", min_waves)
        for n_rec in (1, 3):
            bad_p = params_from_config(cfg)
            bad_p.inv1_mu_log = float("nan")
            counts = torch.full((3, 2), sentinel, dtype=torch.int64, device="cuda")
            rec = (N.McrAssumptions * 3)(N.McrAssumptions(*good), N.McrAssumptions(*good), N.McrAssumptions(*good))
            rc = lib.mcr_probe_assumptions_rng(C.byref(bad_p), C.byref(rng), 0, 0, 1000, 12, rec, n_rec, C.c_void_p(counts.data_ptr()),
                                               0, C.c_void_p(stream))
            assert rc == N.MCR_ERR_INVALID_ARG and "params.inv1_mu_log" in N.last_error(), N.last_error()
            torch.cuda.synchronize()
            assert (counts.cpu() == sentinel).all()
    counts = torch.full((1, 2), sentinel, dtype=torch.int64, device="cuda")
    rc = lib.mcr_probe_assumptions_rng(C.byref(p), C.byref(rng), 0, 0, 1000, 12, None, 0, C.c_void_p(counts.data_ptr()), 0,
                                       C.c_void_p(stream))
    torch.cuda.synchronize()
    assert rc == 0 and (counts.cpu() == sentinel).all()
    with pytest.raises(RuntimeError, match=r"records\[1\]\.equity_inflation_rho"):
        E.probe_assumptions(p, SEED, 0, 0, 100, 12, [good, good[:9] + (-1.5,)])
    assert E.probe_assumptions(p, SEED, 0, 0, 100, 12, []).shape == (0, 2)


@pytest.mark.parametrize("rng", ["philox", "numpy"])
def test_class_probabilities_equal_full_runs(rng):
    cfgd = dict(SCENARIOS["jorge_rho"], seed=4242)
    n, wm = 2000, 150
    scenarios = [{}, {"inv1_returns_mean": 0.02}, {"inflation_rate_mean": 0.08, "inflation_rate_volatility": 0.0},
                 {"equity_inflation_correlation": -0.6, "inv2_premium_over_inflation_mean": 0.0, "monthly_expenses": 2100.25},
                 {"inv1_returns_volatility": 0.35, "initial_balance": 0.0}, {}]
    sim = RetirementMonteCarloSimulator(Config(**cfgd), rng=rng)
    sim.use_final_seeds()
    got = sim.success_probability_by_assumptions(wm, scenarios, n)
    assert got.dtype == np.float64 and got.shape == (len(scenarios),)
    for s, g in zip(scenarios, got):
        ref = RetirementMonteCarloSimulator(Config(**dict(cfgd, **s)), rng=rng)
        ref.use_final_seeds()
        want = ref._success_probability(ref.run_monte_carlo_simulations(wm, n)[0])
        assert g == want, (s, g, want)
    assert len(set(got.tolist())) > 1
    with pytest.raises(ValueError, match=r"scenarios\[0\].*allocation_inv1_pct"):
        sim.success_probability_by_assumptions(wm, [{"allocation_inv1_pct": 0.5}], n)


def test_stress_test_rows():
    cfgd = dict(SCENARIOS["config"], seed=11)
    sim = RetirementMonteCarloSimulator(Config(**cfgd))
    rows = sim.stress_test(240, num_simulations=2000)
    assert len(rows) == 15 and rows[0]["label"] == "base" and rows[0]["overrides"] == {} and rows[0]["delta"] == 0.0
    assert all(set(r) == {"label", "overrides", "probability", "delta"} for r in rows)
    assert all(r["delta"] == r["probability"] - rows[0]["probability"] for r in rows)
    assert rows[0]["probability"] == sim.success_probability_by_assumptions(240, [{}], 2000)[0]
    by = {r["label"]: r for r in rows}
    assert by["equity mean -2 pts"]["delta"] <= by["equity mean -1 pt"]["delta"] <= 0.0 <= by["equity mean +1 pt"]["delta"]
    assert by["inflation mean +2 pts"]["delta"] <= by["inflation mean +1 pt"]["delta"] <= 0.0
    custom = sim.stress_test(240, shifts=[("stagflation", {"inv1_returns_mean": -0.02, "inflation_rate_mean": 0.02})], num_simulations=2000)
    assert [r["label"] for r in custom] == ["base", "stagflation"] and custom[0] == rows[0]
    assert custom[1]["delta"] <= min(by["equity mean -2 pts"]["delta"], by["inflation mean +2 pts"]["delta"])


def test_breakeven_search_on_the_gpu():
    n, wm, field, window, resolution = 5000, 240, "inv1_returns_mean", 0.25, 1e-4
    cfgd = dict(SCENARIOS["config"], seed=99, num_simulations_search=n)
    sim = RetirementMonteCarloSimulator(Config(**cfgd))
    events = []
    value, prob, curve, status = sim.find_breakeven_assumption(wm, field, window=window, resolution=resolution, verbose=False,
                                                               progress_callback=events.append)
    target = cfgd["target_probability"]
    assert status == "found", (value, prob, status)
    assert abs(value / resolution - round(value / resolution)) < 1e-6
    seen = {round(c["value"], 10): c["probability"] for c in curve}
    assert seen[round(value, 10)] == prob
    direct = {}
    for level in (value, round(value - resolution, 10)):   # fresh simulators, search seeds, full runs
        ref = RetirementMonteCarloSimulator(Config(**dict(cfgd, **{field: level})))
        ref.use_search_seeds()
        direct[level] = ref._success_probability(ref.run_monte_carlo_simulations(wm, n)[0])
        assert direct[level] == seen[round(level, 10)]
    assert direct[value] >= target > direct[round(value - resolution, 10)]
    calls = len({e["iteration"] for e in events})
    assert calls <= 1 + math.ceil(math.log(2 * window / resolution) / math.log(16))
    assert {e["type"] for e in events} == {"breakeven_search_iter"}
    assert sim.find_breakeven_assumption(wm, field, window=window, resolution=resolution, verbose=False) == (value, prob, curve, status)
