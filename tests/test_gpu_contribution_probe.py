"""Contribution probes (`mcr_probe_contributions_rng`, `engine.probe_contributions`) and the minimum-contribution search on
the GPU.

The contract: level k's counters equal, bit for bit, those of a count-only launch with monthly_contribution = level k
(`engine.probe_months` of a parameter block that differs only there) — on the contribution fan-out route (Philox, <= 16
streams, tolerance month) and on the per-level route (NumPy stream, longer stream lists, the exact month, or forced)."""

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
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
from test_gpu_expense_probe import SCENARIOS as EXPENSE_SCENARIOS, _cfg

pytestmark = pytest.mark.gpu
SEED = 0xC0_27B1
STRADDLE = 2**32 - 37   # the first wavefront holds paths 2^32 - 37 .. 2^32 + 26 (the producer's general Philox form)

SCENARIOS = {
    "config": EXPENSE_SCENARIOS["config"],
    "jorge_rho": EXPENSE_SCENARIOS["jorge_rho"],
    "no_tax": EXPENSE_SCENARIOS["no_tax"],
    "annual_tax": EXPENSE_SCENARIOS["annual_tax"],
    "contrib_growth": _cfg(contribution_growth_rate_annual=0.07),
    "streams17": EXPENSE_SCENARIOS["streams17"],
    "exact_month": EXPENSE_SCENARIOS["exact_month"],
}


def _levels(base, L):
    """L levels: the scenario's own, 0, a very large one (1e8 a month, the search's cap), duplicates, and a spread."""
    head = [base, 0.0, 1e8, base]
    spread = [round(max(base, 100.0) * (0.2 + 0.17 * k), 2) for k in range(max(0, L - len(head)))]
    return (head + spread)[:L]


def _per_level(p, seed, stream, begin, n, wm, levels):
    out = []
    for x in levels:
        q = params_from_config(Config(**dict(p, monthly_contribution=x)))
        out.append(E.probe_months(q, seed, stream, begin, n, [wm]).cpu().numpy()[0].tolist())
    return out


def _check(cfgd, seed, wm, n, begin, levels, stream=0):
    p = params_from_config(Config(**cfgd))
    got = E.probe_contributions(p, seed, stream, begin, n, wm, levels).cpu().numpy().tolist()
    want = _per_level(cfgd, seed, stream, begin, n, wm, levels)
    assert got == want, (wm, n, begin, len(levels))
    return got


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_counts_equal_plain_launches(name):
    cfgd = SCENARIOS[name]
    Ls = [1, 2, 8, 15, 16, 40]
    i = 0
    for wm in (0, 1, 13, 233):
        for n in (1, 63, 65, 50_000):
            begin = (0, 12_345)[i % 2]
            L = Ls[i % len(Ls)]
            i += 1
            got = _check(cfgd, SEED, wm, n, begin, _levels(cfgd["monthly_contribution"], L))
            assert all(c[1] == n for c in got)
            if wm == 0:   # nothing is ever contributed
                assert len({c[0] for c in got}) == 1
            elif L >= 3 and n >= 1000:
                assert got[2][0] >= got[1][0]   # 1e8 a month against nothing


def test_counts_with_the_numpy_stream():
    cfgd = SCENARIOS["config"]
    for wm, n, L in ((0, 65, 2), (13, 1000, 8), (233, 5000, 16)):
        rng = N.numpy_rng(1234, child_offset=0)
        _check(cfgd, rng, wm, n, 0, _levels(cfgd["monthly_contribution"], L), stream=1)


@pytest.mark.parametrize("name", ["config", "jorge_rho"])
def test_counts_at_a_million_paths(name):
    cfgd = SCENARIOS[name]
    for L in (8, 16):
        _check(cfgd, SEED, 240, 1_000_000, 12_345, _levels(cfgd["monthly_contribution"], L))


def test_counts_straddling_2_pow_32():
    cfgd = SCENARIOS["config"]
    for n, L in ((65, 3), (20_000, 8)):
        _check(cfgd, SEED, 233, n, STRADDLE, _levels(cfgd["monthly_contribution"], L))


def test_forced_per_level_route_agrees(monkeypatch):
    cfgd = SCENARIOS["config"]
    p = params_from_config(Config(**cfgd))
    levels = _levels(cfgd["monthly_contribution"], 15)
    monkeypatch.setenv("MCR_CONTRIBUTION_FANOUT_MIN_WAVES", "0")
    fan = E.probe_contributions(p, SEED, 0, 0, 50_000, 240, levels).cpu().numpy()
    monkeypatch.setenv("MCR_CONTRIBUTION_FANOUT_MIN_WAVES", str(2**40))
    per = E.probe_contributions(p, SEED, 0, 0, 50_000, 240, levels).cpu().numpy()
    assert fan.tolist() == per.tolist()


def test_permuting_levels_permutes_counts():
    cfgd = SCENARIOS["jorge_rho"]
    p = params_from_config(Config(**cfgd))
    levels = [round(100.0 * 1.6 ** k, 2) for k in range(12)]
    perm = np.random.default_rng(3).permutation(len(levels))
    a = E.probe_contributions(p, SEED, 0, 0, 20_000, 120, levels).cpu().numpy()
    b = E.probe_contributions(p, SEED, 0, 0, 20_000, 120, [levels[i] for i in perm]).cpu().numpy()
    assert b.tolist() == a[perm].tolist()
    assert a[0, 0] < a[-1, 0]   # the spread reaches from fewer to more successes


def test_invalid_levels_leave_counts_untouched():
    import torch

    p = params_from_config(Config(**SCENARIOS["config"]))
    lib = N.load_library()
    rng = N.McrRng()
    rng.kind, rng.philox_seed = N.MCR_RNG_PHILOX, SEED
    stream = torch.cuda.current_stream(0).cuda_stream
    sentinel = -0x1234_5678
    for bad in (float("nan"), -0.01, float("inf")):
        counts = torch.full((3, 2), sentinel, dtype=torch.int64, device="cuda")
        lv = (C.c_double * 3)(1000.0, bad, 2000.0)
        rc = lib.mcr_probe_contributions_rng(C.byref(p), C.byref(rng), 0, 0, 1000, 12, lv, 3, C.c_void_p(counts.data_ptr()),
                                             0, C.c_void_p(stream))
        assert rc == -1 and "monthly_contribution[1]" in N.last_error()
        torch.cuda.synchronize()
        assert (counts.cpu() == sentinel).all()
    counts = torch.full((1, 2), sentinel, dtype=torch.int64, device="cuda")
    rc = lib.mcr_probe_contributions_rng(C.byref(p), C.byref(rng), 0, 0, 1000, 12, None, 0, C.c_void_p(counts.data_ptr()), 0,
                                         C.c_void_p(stream))
    torch.cuda.synchronize()
    assert rc == 0 and (counts.cpu() == sentinel).all()
    with pytest.raises(RuntimeError, match="monthly_contribution"):
        E.probe_contributions(p, SEED, 0, 0, 100, 12, [1.0, float("nan")])
    assert E.probe_contributions(p, SEED, 0, 0, 100, 12, []).shape == (0, 2)


@pytest.mark.parametrize("rng", ["philox", "numpy"])
@pytest.mark.parametrize("stream", ["search", "final"])
def test_class_probabilities_equal_full_runs(rng, stream):
    cfgd = dict(SCENARIOS["jorge_rho"], seed=4242)
    n, wm = 3000, 150
    levels = [2500.0, 0.0, 4100.5, 2500.0]
    sim = RetirementMonteCarloSimulator(Config(**cfgd), rng=rng)
    (sim.use_search_seeds if stream == "search" else sim.use_final_seeds)()
    got = sim.success_probability_by_contributions(wm, levels, n)
    assert got.dtype == np.float64 and got.shape == (len(levels),)
    for x, g in zip(levels, got):
        ref = RetirementMonteCarloSimulator(Config(**dict(cfgd, monthly_contribution=x)), rng=rng)
        (ref.use_search_seeds if stream == "search" else ref.use_final_seeds)()
        want = ref._success_probability(ref.run_monte_carlo_simulations(wm, n)[0])
        assert g == want, (x, g, want)


@pytest.mark.parametrize("name,wm,n", [("config", 120, 20_000), ("jorge_rho", 96, 20_000)])
def test_search_on_the_gpu(name, wm, n):
    cfgd = dict(SCENARIOS[name], seed=99, num_simulations_search=n)
    sim = RetirementMonteCarloSimulator(Config(**cfgd))
    events = []
    x, prob, curve = sim.find_minimum_monthly_contribution(wm, verbose=False, progress_callback=events.append)
    target = cfgd["target_probability"]
    seen = {c["monthly_contribution"]: c["probability"] for c in curve}
    assert seen[0.0] < target, "level 0 must miss for this test to search"
    assert x > 0 and x == round(x, 2)
    lo = max(v for v in seen if v < x)
    assert x - lo <= 1.0 + 1e-9
    assert seen[x] == prob >= target > seen[lo]
    for level, hit in ((x, True), (lo, False)):   # fresh simulators, search seeds, full runs
        ref = RetirementMonteCarloSimulator(Config(**dict(cfgd, monthly_contribution=level)))
        ref.use_search_seeds()
        pr = ref._success_probability(ref.run_monte_carlo_simulations(wm, n)[0])
        assert pr == seen[level] and (pr >= target) == hit
    # probe calls: the bracket, then ceil(log_{L+1}(range / resolution)) refinements
    calls = sorted({e["iteration"] for e in events})
    bracket = len({e["iteration"] for e in events if e["lo"] is None})
    first_refine = next((e for e in events if e["lo"] is not None), None)
    refine_bound = 0
    if first_refine:
        rng_w = first_refine["hi"] - first_refine["lo"]
        refine_bound = math.ceil(math.log(rng_w / 1.0) / math.log(N.MCR_MAX_EXPENSE_FANOUT + 1) - 1e-12)
    assert len(calls) <= bracket + refine_bound
    assert {e["type"] for e in events} == {"contribution_search_iter"}
    assert sim.find_minimum_monthly_contribution(wm, verbose=False) == (x, prob, curve)   # deterministic


def test_search_at_zero_working_months_probes_level_zero_once():
    cfgd = dict(SCENARIOS["config"], seed=99, num_simulations_search=5000)
    sim = RetirementMonteCarloSimulator(Config(**cfgd))
    x, prob, curve = sim.find_minimum_monthly_contribution(0, verbose=False)
    assert [c["monthly_contribution"] for c in curve] == [0.0] and curve[0]["probability"] == prob
    assert x == (0.0 if prob >= cfgd["target_probability"] else -1.0)


def test_cli_min_contribution():
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--seed", "7", "--working-months", "120", "--search-paths", "5000",
           "--min-contribution"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"scenario", "rng", "working_months", "target_probability", "min_monthly_contribution", "probability",
                        "probes", "curve", "seconds"}
    assert out["working_months"] == 120 and out["rng"] == "philox"
    assert out["min_monthly_contribution"] > 0 and out["probability"] >= out["target_probability"]
    assert out["probes"] >= 1 and out["curve"] and {"monthly_contribution", "probability"} <= set(out["curve"][0])
