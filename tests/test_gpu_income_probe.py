"""Income probes (`mcr_probe_income_rng`, `engine.probe_income`) and the required-income search on the GPU.

The contract: option k's counters equal, bit for bit, those of a count-only launch with (initial_balance,
monthly_contribution, monthly_expenses) and (monthly_amount_today, start_at_age, duration_years) of ONE income stream = option
k (`engine.probe_months` of a parameter block that differs only there) — on the income fan-out route (Philox, <= 16 kept
streams, tolerance month) and on the per-option route (NumPy stream, longer stream lists, the exact month, or forced).
`mcr_probe_income_last_fanout_launches` proves which route ran."""

from __future__ import annotations

import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.income import INCOME_OPTION_FIELDS
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
from test_gpu_scenario_probe import FROZEN8, SCENARIOS, _cfg, _stream

pytestmark = pytest.mark.gpu
SEED = 0x1C0_4E57
STRADDLE = 2**32 - 37   # the first wavefront holds paths 2^32 - 37 .. 2^32 + 26 (the producer's general Philox form)
MONEY = INCOME_OPTION_FIELDS[:3]
STREAM_FIELDS = INCOME_OPTION_FIELDS[3:]

#: five streams, frozen at the odd indices (`_stream`): every one pays, so kept record k is list entry k
FIVE = _cfg(other_income_streams=[_stream(i) for i in range(5)])
#: ... with entries 0 and 3 paying nothing: the plain launch drops them, so list entry 4 is kept record 2 of three when it is
#: probed, and entry 3 (frozen, own amount 0) is kept record 2 of four
FIVE_ZEROS = _cfg(other_income_streams=[dict(_stream(i), monthly_amount_today=0.0 if i in (0, 3) else 40.0 + 7 * i) for i in range(5)])

#: name -> (config, probed list index, the fan-out route runs).  config.json's list is [a paying indexed pension, a frozen
#: rental income that pays 0].
CASES = {
    # kept record 0 (S0), in every compiled tax / annual variant
    "config_s0": (SCENARIOS["config"], 0, True),
    "jorge_rho_s0": (SCENARIOS["jorge_rho"], 0, True),
    "no_tax_s0": (SCENARIOS["no_tax"], 0, True),
    "annual_tax_s0": (SCENARIOS["annual_tax"], 0, True),
    "contrib_growth_s0": (SCENARIOS["contrib_growth"], 0, True),
    # kept record 1 (S1): a frozen stream whose own amount is 0 while the other pays
    "config_s1_frozen_zero": (SCENARIOS["config"], 1, True),
    "five_s0": (FIVE, 0, True),                    # kept record 0 of five, indexed
    "five_s1_frozen": (FIVE, 1, True),             # kept record 1 of five, frozen
    "five_s2": (FIVE, 2, True),                    # kept record 2 of five, indexed: substituted in the stream loop
    "five_s3_frozen": (FIVE, 3, True),             # kept record 3 of five, frozen: its lock column per wave
    "five_zeros_s3_frozen_zero": (FIVE_ZEROS, 3, True),   # own amount 0, frozen, behind a dropped entry: kept record 2 of four
    "five_zeros_s4": (FIVE_ZEROS, 4, True),        # list entry 4 = kept record 2 of three
    "five_zeros_s0_zero": (FIVE_ZEROS, 0, True),   # own amount 0, indexed, first of the list
    # per-option route
    "streams17_s3": (SCENARIOS["streams17"], 3, False),
    "streams17_s16": (SCENARIOS["streams17"], 16, False),    # the entry behind mcr_params.extra_streams
    "exact_month_s0": (SCENARIOS["exact_month"], 0, False),
}


def _horizon_age(cfgd, wm):
    return cfgd["current_age"] + wm / 12.0 + cfgd["retirement_years"]


def _options(cfgd, idx, L):
    """L options (a prefix of the list, so from L = 8 on all of these): the config's own six values; amount 0; a start below
    current_age (clamps to retirement); a start beyond the horizon of every month of the sweep (the stream never pays);
    duration 0 (never pays) and 1; a duplicate of the first; then a spread in which all six fields differ."""
    s = cfgd["other_income_streams"][idx]
    money = tuple(float(cfgd[f]) for f in MONEY)
    own = money + (float(s["monthly_amount_today"]), float(s["start_at_age"]), s["duration_years"])
    amount = max(own[3], 500.0)
    assert _horizon_age(cfgd, 233) < 120.0 and cfgd["current_age"] > 20.0
    head = [own, money + (0.0, own[4], own[5]), money + (amount, 20.0, own[5]), money + (amount, 120.0, None),
            money + (amount, own[4], 0), money + (amount * 3, cfgd["current_age"] + 1.0, 1), own]
    spread = [(round(max(money[0], 1000.0) * (0.1 + 0.9 * k), 2), round(max(money[1], 100.0) * (2.5 - 0.07 * k), 2),
               round(max(money[2], 100.0) * (0.4 + 0.09 * k), 2), round(amount * (0.2 + 0.37 * k), 2),
               min(120.0, cfgd["current_age"] - 3.0 + 2.75 * k), [None, 3, 7, 15, 30][k % 5] if k else 11) for k in range(max(0, L - len(head)))]
    return (head + spread)[:L]


def _replaced(cfgd, idx, option):
    streams = [dict(s) for s in cfgd["other_income_streams"]]
    streams[idx].update(zip(STREAM_FIELDS, option[3:]))
    return dict(cfgd, other_income_streams=streams, **dict(zip(MONEY, option[:3])))


_REFERENCE = {}   # (config, stream, seed, stream id, path range, month, option) -> counters of the plain launch: computed once, shared


def _plain(cfgd, idx, seed, stream, begin, n, wm, option):
    q = params_from_config(Config(**_replaced(cfgd, idx, option)))
    if not isinstance(seed, int):   # (a NumPy-stream descriptor: three small cases, not shared)
        return E.probe_months(q, seed, stream, begin, n, [wm]).cpu().numpy()[0].tolist()
    key = (json.dumps(cfgd, sort_keys=True, default=str), idx, seed, stream, begin, n, wm, option)
    if key not in _REFERENCE:
        _REFERENCE[key] = E.probe_months(q, seed, stream, begin, n, [wm]).cpu().numpy()[0].tolist()
    return _REFERENCE[key]


def _launches():
    return N.load_library().mcr_probe_income_last_fanout_launches()


def _check(cfgd, idx, seed, wm, n, begin, options, stream=0, fanout=None):
    p = params_from_config(Config(**cfgd))
    got = E.probe_income(p, seed, stream, begin, n, wm, idx, options).cpu().numpy().tolist()
    launches = _launches()
    want = [_plain(cfgd, idx, seed, stream, begin, n, wm, o) for o in options]
    assert got == want, (idx, wm, n, begin, len(options))
    if fanout is not None:
        if fanout and len(options) >= 2:
            assert launches >= 1, (idx, wm, n, begin, len(options))
        else:
            assert launches == 0, (idx, wm, n, begin, len(options))
    return got


def _sweep(cfgd, idx, fanout):
    Ls = [1, 2, 8, 15, 16, 40]
    i = 0
    for wm in (0, 1, 13, 233):
        for n in (1, 63, 65, 50_000):
            begin = (0, 12_345)[i % 2]
            L = Ls[i % len(Ls)]
            i += 1
            got = _check(cfgd, idx, SEED, wm, n, begin, _options(cfgd, idx, L), fanout=fanout)
            assert all(c[1] == n for c in got)
            if L >= 8:
                assert got[6] == got[0]                       # the duplicate
                assert got[3] == got[4]                       # never paying, two ways: beyond the horizon, duration 0


@pytest.mark.parametrize("name", list(CASES))
def test_counts_equal_plain_launches(name):
    cfgd, idx, fanout = CASES[name]
    _sweep(cfgd, idx, fanout)


def test_options_cover_the_cases_the_contract_names():
    """The option list of the sweep, read back through the host derivation the library uses."""
    cfgd, idx, _ = CASES["five_s3_frozen"]
    opts = _options(cfgd, idx, 40)
    assert len(opts) == 40 and opts[6] == opts[0]
    for wm in (0, 1, 13, 233):
        months = cfgd["retirement_years"] * 12
        assert E.stream_start_month_index(cfgd["current_age"], wm, opts[2][4]) == 0            # clamps to retirement
        assert E.stream_start_month_index(cfgd["current_age"], wm, opts[3][4]) >= months       # never pays
    assert opts[1][3] == 0.0 and opts[4][5] == 0 and opts[5][5] == 1
    for f in range(6):
        assert len({o[f] for o in opts[7:]}) > 1
    assert all(0.0 <= o[4] <= 120.0 for o in opts)


def test_counts_with_fewer_records_per_launch_than_fifteen():
    """Eight frozen streams = 8 lock columns per consumer wave: a launch takes 11 options."""
    _sweep(FROZEN8, 5, True)
    lib = N.load_library()
    for L, launches in ((11, 1), (12, 2), (15, 2), (40, 4)):   # one full launch, 6 + 6, 8 + 7, 4 x 10
        _check(FROZEN8, 3, SEED, 120, 2000, 77, _options(FROZEN8, 3, L), fanout=True)
        assert lib.mcr_probe_income_last_fanout_launches() == launches   # (the plain launches of the check are not probe calls)


def test_money_only_options_equal_the_scenario_probe():
    for name, idx in (("jorge_rho", 0), ("config", 1)):
        cfgd = SCENARIOS[name]
        p = params_from_config(Config(**cfgd))
        s = cfgd["other_income_streams"][idx]
        own = (float(s["monthly_amount_today"]), float(s["start_at_age"]), s["duration_years"])
        scenarios = [tuple(float(cfgd[f]) for f in MONEY), (0.0, 0.0, 0.0)] + \
                    [(round(20000.0 * 1.7 ** k, 2), round(3000.0 - 200.0 * k, 2), round(2500.0 + 150.0 * k, 2)) for k in range(13)]
        for wm, n in ((0, 65), (150, 20_000)):
            a = E.probe_income(p, SEED, 0, 5, n, wm, idx, [sc + own for sc in scenarios]).cpu().numpy().tolist()
            assert _launches() >= 1
            assert a == E.probe_scenarios(p, SEED, 0, 5, n, wm, scenarios).cpu().numpy().tolist()


def test_counts_with_the_numpy_stream():
    cfgd, idx = FIVE, 3
    for wm, n, L in ((0, 65, 2), (13, 1000, 8), (233, 5000, 16)):
        rng = N.numpy_rng(1234, child_offset=0)
        _check(cfgd, idx, rng, wm, n, 0, _options(cfgd, idx, L), stream=1, fanout=False)


def test_counts_straddling_2_pow_32():
    for name in ("config_s0", "five_s3_frozen"):
        cfgd, idx, _ = CASES[name]
        for n, L in ((65, 3), (20_000, 8)):
            _check(cfgd, idx, SEED, 233, n, STRADDLE, _options(cfgd, idx, L), fanout=True)


def test_forced_per_option_route_agrees(monkeypatch):
    for name in ("config_s0", "five_s3_frozen"):
        cfgd, idx, _ = CASES[name]
        p = params_from_config(Config(**cfgd))
        options = _options(cfgd, idx, 15)
        monkeypatch.setenv("MCR_INCOME_FANOUT_MIN_WAVES", "0")
        fan = E.probe_income(p, SEED, 0, 0, 50_000, 240, idx, options).cpu().numpy()
        assert _launches() == 1
        monkeypatch.setenv("MCR_INCOME_FANOUT_MIN_WAVES", str(2**40))
        per = E.probe_income(p, SEED, 0, 0, 50_000, 240, idx, options).cpu().numpy()
        assert _launches() == 0
        assert fan.tolist() == per.tolist()


def test_permuting_options_permutes_counts():
    cfgd, idx, _ = CASES["five_s2"]
    p = params_from_config(Config(**cfgd))
    money = tuple(float(cfgd[f]) for f in MONEY)
    options = [money + (round(300.0 * 1.6 ** k, 2), 45.0 + 2.5 * k, [None, 4, 9, 20][k % 4]) for k in range(12)]
    perm = np.random.default_rng(3).permutation(len(options))
    a = E.probe_income(p, SEED, 0, 0, 20_000, 120, idx, options).cpu().numpy()
    b = E.probe_income(p, SEED, 0, 0, 20_000, 120, idx, [options[i] for i in perm]).cpu().numpy()
    assert b.tolist() == a[perm].tolist()
    assert len({int(x) for x in a[:, 0]}) > 1   # the options do differ in their counts


def test_invalid_options_leave_counts_untouched():
    import torch

    p = params_from_config(Config(**SCENARIOS["config"]))
    lib = N.load_library()
    rng = N.McrRng()
    rng.kind, rng.philox_seed = N.MCR_RNG_PHILOX, SEED
    stream = torch.cuda.current_stream(0).cuda_stream
    sentinel = -0x1234_5678

    def call(options, index, n_options=None):
        counts = torch.full((3, 2), sentinel, dtype=torch.int64, device="cuda")
        rc = lib.mcr_probe_income_rng(C.byref(p), C.byref(rng), 0, 0, 1000, 12, index, options,
                                      len(options) if n_options is None else n_options, C.c_void_p(counts.data_ptr()), 0,
                                      C.c_void_p(stream))
        msg = N.last_error()
        torch.cuda.synchronize()
        return rc, msg, bool((counts.cpu() == sentinel).all())

    def good():
        return (N.McrIncomeOption * 3)(N.McrIncomeOption(1000.0, 10.0, 20.0, 500.0, 62.0, -1, 0),
                                       N.McrIncomeOption(1000.0, 10.0, 20.0, 700.0, 67.0, 10, 0),
                                       N.McrIncomeOption(2000.0, 0.0, 5.0, 0.0, 0.0, 0, 0))

    rc, msg, untouched = call(good(), 0)
    assert rc == 0 and not untouched
    cases = [(f, bad) for f in INCOME_OPTION_FIELDS[:5] for bad in (float("nan"), -0.01, float("inf"))]
    cases += [("start_at_age", 121.0), ("duration_years", -2), ("reserved", 1)]
    for field, bad in cases:
        op = good()
        setattr(op[1], field, bad)
        rc, msg, untouched = call(op, 0)
        assert rc == -1 and f"options[1].{field}" in msg, (field, bad, msg)
        assert untouched, (field, bad)
        assert lib.mcr_probe_income_last_fanout_launches() == 0
    for index in (-1, p.n_streams):
        rc, msg, untouched = call(good(), index)
        assert rc == -1 and "stream_index" in msg and untouched, (index, msg)
    rc, msg, untouched = call(good(), 0, n_options=0)
    assert rc == 0 and untouched
    with pytest.raises(RuntimeError, match=r"options\[1\]\.start_at_age"):
        E.probe_income(p, SEED, 0, 0, 100, 12, 0, [(1.0, 1.0, 1.0, 1.0, 60.0, None), (1.0, 1.0, 1.0, 1.0, float("nan"), 3)])
    with pytest.raises(ValueError):
        E.probe_income(p, SEED, 0, 0, 100, 12, 0, [(1.0, 1.0, 1.0)])
    assert E.probe_income(p, SEED, 0, 0, 100, 12, 0, []).shape == (0, 2)


OPTION_MAPS = [{}, {"monthly_amount_today": 0.0}, {"start_at_age": 62.0, "monthly_amount_today": 5880.0},
               {"start_at_age": 70.0, "monthly_amount_today": 10416.0, "duration_years": 12},
               {"initial_balance": 250000.0, "monthly_contribution": 0.0, "monthly_expenses": 2100.25, "duration_years": None}, {}]


def _config_with(cfgd, idx, option_map):
    streams = [dict(s) for s in cfgd["other_income_streams"]]
    streams[idx].update({k: v for k, v in option_map.items() if k in STREAM_FIELDS})
    return dict(cfgd, other_income_streams=streams, **{k: v for k, v in option_map.items() if k in MONEY})


@pytest.mark.parametrize("rng", ["philox", "numpy"])
@pytest.mark.parametrize("stream", ["search", "final"])
def test_class_probabilities_equal_full_runs(rng, stream):
    cfgd = dict(SCENARIOS["jorge_rho"], seed=4242)
    n, wm = 3000, 150
    sim = RetirementMonteCarloSimulator(Config(**cfgd), rng=rng)
    (sim.use_search_seeds if stream == "search" else sim.use_final_seeds)()
    got = sim.success_probability_by_income_options(wm, "State Pension", OPTION_MAPS, n)
    assert (_launches() >= 1) if rng == "philox" else (_launches() == 0)
    assert got.dtype == np.float64 and got.shape == (len(OPTION_MAPS),)
    for o, g in zip(OPTION_MAPS, got):
        ref = RetirementMonteCarloSimulator(Config(**_config_with(cfgd, 0, o)), rng=rng)
        (ref.use_search_seeds if stream == "search" else ref.use_final_seeds)()
        want = ref._success_probability(ref.run_monte_carlo_simulations(wm, n)[0])
        assert g == want, (o, g, want)
    with pytest.raises(ValueError, match="tax_rate"):
        sim.success_probability_by_income_options(wm, 0, [{"tax_rate": 0.5}], n)


def test_compare_claiming_options_picks_the_argmax():
    cfgd = dict(SCENARIOS["config"], seed=11)
    sim = RetirementMonteCarloSimulator(Config(**cfgd))
    sim.use_final_seeds()
    options = [{"start_at_age": 62.0, "monthly_amount_today": 2800.0}, {"start_at_age": 67.0, "monthly_amount_today": 4000.0},
               {"start_at_age": 67.0, "monthly_amount_today": 4000.0}, {"start_at_age": 70.0, "monthly_amount_today": 1000.0}]
    table = sim.compare_claiming_options(240, "State Pension", options, 3000)
    probs = sim.success_probability_by_income_options(240, 0, options, 3000)
    assert table["stream"] == 0 and len(table["options"]) == 4
    assert [r["probability"] for r in table["options"]] == probs.tolist()
    assert all(set(r) == set(INCOME_OPTION_FIELDS) | {"probability"} for r in table["options"])
    assert [(r["start_at_age"], r["monthly_amount_today"], r["duration_years"]) for r in table["options"]] == \
        [(62.0, 2800.0, None), (67.0, 4000.0, None), (67.0, 4000.0, None), (70.0, 1000.0, None)]
    assert table["best"] == int(np.argmax(probs))          # (np.argmax: the first of equals)
    assert probs[1] == probs[2]
    assert len(set(probs.tolist())) > 1


def _call_bound(events):
    """probe calls: the bracket, then ceil(log_{L+1}(range / resolution)) refinements"""
    bracket = len({e["iteration"] for e in events if e["lo"] is None})
    first_refine = next((e for e in events if e["lo"] is not None), None)
    refine_bound = 0
    if first_refine:
        rng_w = first_refine["hi"] - first_refine["lo"]
        refine_bound = math.ceil(math.log(rng_w / 1.0) / math.log(N.MCR_MAX_EXPENSE_FANOUT + 1) - 1e-12)
    return bracket + refine_bound


def test_search_on_the_gpu():
    """How large a pension, paid from the first month of retirement on, does retiring after ten years take?  (Above 10 000 /
    0.725 a month it covers the spending whatever the market does, so the target is reachable.)"""
    n, wm = 20_000, 120
    cfgd = dict(SCENARIOS["config"], seed=99, num_simulations_search=n)
    sim = RetirementMonteCarloSimulator(Config(**cfgd))
    events = []
    x, prob, curve = sim.find_minimum_income_amount(wm, "State Pension", start_at_age=0.0, verbose=False, progress_callback=events.append)
    target = cfgd["target_probability"]
    seen = {c["monthly_amount_today"]: c["probability"] for c in curve}
    assert seen[0.0] < target, "level 0 must miss for this test to search"
    assert 0 < x <= 13793.11 and x == round(x, 2)
    lo = max(v for v in seen if v < x)
    assert x - lo <= 1.0 + 1e-9
    assert seen[x] == prob >= target > seen[lo]
    for level, hit in ((x, True), (lo, False)):   # fresh simulators, search seeds, full runs
        ref = RetirementMonteCarloSimulator(Config(**_config_with(cfgd, 0, {"monthly_amount_today": level, "start_at_age": 0.0})))
        ref.use_search_seeds()
        pr = ref._success_probability(ref.run_monte_carlo_simulations(wm, n)[0])
        assert pr == seen[level] and (pr >= target) == hit
    assert len({e["iteration"] for e in events}) <= _call_bound(events)
    assert {e["type"] for e in events} == {"income_amount_search_iter"}
    assert sim.find_minimum_income_amount(wm, 0, start_at_age=0.0, verbose=False) == (x, prob, curve)   # deterministic


def _cli(*extra):
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--seed", "7", "--search-paths", "5000", *extra]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_cli_income_options():
    out = _cli("--paths", "5000", "--working-months", "240", "--income-options", "State Pension", "--claim-ages", "62,67,70",
               "--claim-amounts", "1400,2000,2480")
    assert set(out) == {"scenario", "rng", "working_months", "num_simulations", "target_probability", "stream", "options", "best",
                        "seconds"}
    assert out["stream"] == 0 and out["working_months"] == 240 and out["num_simulations"] == 5000 and out["rng"] == "philox"
    assert [(o["start_at_age"], o["monthly_amount_today"]) for o in out["options"]] == [(62.0, 1400.0), (67.0, 2000.0), (70.0, 2480.0)]
    assert all(set(o) == set(INCOME_OPTION_FIELDS) | {"probability"} for o in out["options"])
    probs = [o["probability"] for o in out["options"]]
    assert out["best"] == probs.index(max(probs))


def test_cli_min_income():
    out = _cli("--working-months", "120", "--min-income", "0", "--claim-age", "50")
    assert set(out) == {"scenario", "rng", "working_months", "stream", "start_at_age", "target_probability", "min_income_amount",
                        "probability", "probes", "curve", "seconds"}
    assert out["working_months"] == 120 and out["stream"] == 0 and out["start_at_age"] == 50.0
    assert out["min_income_amount"] > 0 and out["probability"] >= out["target_probability"]
    assert out["probes"] >= 1 and out["curve"] and set(out["curve"][0]) == {"monthly_amount_today", "probability"}
