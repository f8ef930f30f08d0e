"""The allocation methods of `RetirementMonteCarloSimulator` on the GPU: `success_probability_by_allocations` against full runs
of simulators whose config differs only in the split, `compare_allocations` with and without the paired and outcome keys,
`find_best_allocation` against the probabilities of its own points, and two ranks on one card against the single process."""

from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from allocation_dist_worker import N_PATHS as DIST_PATHS, SPLITS, WM, make_simulator as _sim
from conftest import REPO
from monte_carlo_retirement_amd import Config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.allocation import ALLOCATION_OPTION_FIELDS, DEFAULT_ALLOCATIONS
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
from test_gpu_expense_probe import SCENARIOS

pytestmark = pytest.mark.gpu
DIFFERENCE_KEYS = {"delta", "se", "se_unpaired", "p_value", "rescued"}
OUTCOME_KEYS = {"lasts_until_age", "median_ruin_age", "final_balance"}


@pytest.mark.parametrize("rng", ["philox", "numpy"])
@pytest.mark.parametrize("stream", ["search", "final"])
def test_class_probabilities_equal_full_runs(rng, stream):
    cfgd = dict(SCENARIOS["jorge_rho"], seed=4242)
    n, wm = 3000, 150
    options = [float(cfgd["allocation_inv1_pct"]), 0.0, 1.0, 0.35, {"allocation_inv1_pct": 0.8, "monthly_expenses": 3333.0},
               {"allocation_inv1_pct": 0.2, "initial_balance": 250000.0, "monthly_contribution": 0.0}, 0.35]
    sim = RetirementMonteCarloSimulator(Config(**cfgd), rng=rng)
    (sim.use_search_seeds if stream == "search" else sim.use_final_seeds)()
    got = sim.success_probability_by_allocations(wm, options, n)
    assert got.dtype == np.float64 and got.shape == (len(options),)
    for o, g in zip(options, got):
        over = o if isinstance(o, dict) else {"allocation_inv1_pct": o}
        ref = RetirementMonteCarloSimulator(Config(**dict(cfgd, **over)), rng=rng)
        (ref.use_search_seeds if stream == "search" else ref.use_final_seeds)()
        want = ref._success_probability(ref.run_monte_carlo_simulations(wm, n)[0])
        assert g == want, (o, g, want)
    with pytest.raises(ValueError, match=r"allocations\[1\]\.allocation_inv1_pct"):
        sim.success_probability_by_allocations(wm, [0.5, 1.5], n)
    with pytest.raises(ValueError, match="inv1_returns_mean"):
        sim.success_probability_by_allocations(wm, [{"allocation_inv1_pct": 0.5, "inv1_returns_mean": 0.1}], n)
    assert sim.success_probability_by_allocations(wm, [], n).shape == (0,)
    assert sim.joint_outcomes_by_allocations(wm, options, n).probabilities.tobytes() == got.tobytes()
    assert sim.option_outcomes_by_allocations(wm, options, n).probabilities.tobytes() == got.tobytes()


def test_compare_documents_extend_the_plain_one():
    sim, n = _sim(), 3000
    plain = sim.compare_allocations(WM, SPLITS, n)
    assert set(plain) == {"options", "best"} and len(plain["options"]) == len(SPLITS)
    assert all(set(r) == set(ALLOCATION_OPTION_FIELDS) | {"probability"} for r in plain["options"])
    assert [r["allocation_inv1_pct"] for r in plain["options"]] == [0.0, 0.3, 0.6, 0.6, 1.0, 0.45]
    assert plain["options"][5]["monthly_expenses"] == 7000.0 and plain["options"][2] == plain["options"][3]
    probs = [r["probability"] for r in plain["options"]]
    assert probs == sim.success_probability_by_allocations(WM, SPLITS, n).tolist()
    assert plain["best"] == probs.index(max(probs))                              # the first of equals
    both = sim.compare_allocations(WM, SPLITS, n, paired=True, outcomes=True)
    assert set(both) == set(plain) | {"tied_with_best", "all_succeed", "none_succeed"}
    added = OUTCOME_KEYS | {"vs_best"}
    stripped = dict({k: v for k, v in both.items() if k in plain}, options=[{k: v for k, v in r.items() if k not in added} for r in both["options"]])
    assert stripped == plain
    assert all(set(r) == set(ALLOCATION_OPTION_FIELDS) | {"probability"} | added for r in both["options"])
    best = both["best"]
    assert both["options"][best]["vs_best"]["delta"] == 0.0 and best in both["tied_with_best"]
    for r in both["options"]:
        assert set(r["vs_best"]) == DIFFERENCE_KEYS and r["vs_best"]["delta"] >= 0.0
        assert set(r["lasts_until_age"]) == {"90", "95", "99"} and set(r["final_balance"]) == {"p5", "p25", "p50", "p75", "p95"}
    assert both["options"][2]["vs_best"] == both["options"][3]["vs_best"]        # the duplicate
    paired = sim.compare_allocations(WM, SPLITS, n, paired=True)
    assert dict(both, options=[{k: v for k, v in r.items() if k not in OUTCOME_KEYS} for r in both["options"]]) == paired
    # the default: the eleven splits 0, 0.1, ..., 1
    default = sim.compare_allocations(WM, num_simulations=n)
    assert [r["allocation_inv1_pct"] for r in default["options"]] == list(DEFAULT_ALLOCATIONS) == [i / 10.0 for i in range(11)]
    assert [r["probability"] for r in default["options"]] == sim.success_probability_by_allocations(WM, DEFAULT_ALLOCATIONS, n).tolist()


@pytest.mark.parametrize("rng,n", [("philox", 20_000), ("numpy", 1500)])
def test_find_best_allocation(rng, n):
    cfgd = dict(SCENARIOS["config"], seed=99, num_simulations_search=n)
    own = float(cfgd["allocation_inv1_pct"])
    sim = RetirementMonteCarloSimulator(Config(**cfgd), rng=rng)
    events = []
    best, prob, curve, tied = sim.find_best_allocation(WM, verbose=False, progress_callback=events.append)
    points = [c["allocation_inv1_pct"] for c in curve]
    assert len(set(points)) == len(points) and points[:11] == [i / 10.0 for i in range(11)]
    assert all(p == round(p, 2) and 0.0 <= p <= 1.0 for p in points)
    rounds = [e["iteration"] for e in events]
    assert [e["allocation_inv1_pct"] for e in events] == points and max(rounds) == 3
    assert all(rounds.count(r) <= N.MCR_MAX_EXPENSE_FANOUT for r in set(rounds))
    assert {e["type"] for e in events} == {"allocation_search_iter"}
    # the curve is what the probe says of the same points on the search stream
    check = RetirementMonteCarloSimulator(Config(**cfgd), rng=rng)
    check.use_search_seeds()
    assert [c["probability"] for c in curve] == check.success_probability_by_allocations(WM, points, n).tolist()
    # the answer is the curve's maximum under the tie rule, and tied holds it
    seen = {c["allocation_inv1_pct"]: c["probability"] for c in curve}
    assert best == min(seen, key=lambda s: (-seen[s], abs(round(100 * s) - round(100 * own)), s)) and prob == seen[best]   # (0.6: whole hundredths)
    assert best in tied and set(tied) <= set(points[:11]) | {best}
    joint = check.joint_outcomes_by_allocations(WM, sorted(set(points[:11]) | {best}), n)
    assert tied == [sorted(set(points[:11]) | {best})[j] for j in joint.indistinguishable_from(sorted(set(points[:11]) | {best}).index(best))]
    # a full run at the answer, on a fresh simulator with the search seeds
    ref = RetirementMonteCarloSimulator(Config(**dict(cfgd, allocation_inv1_pct=best)), rng=rng)
    ref.use_search_seeds()
    assert ref._success_probability(ref.run_monte_carlo_simulations(WM, n)[0]) == prob
    assert sim.find_best_allocation(WM, verbose=False) == (best, prob, curve, tied)   # deterministic


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_return_the_single_process_document(tmp_path):
    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                       os.path.join(REPO, "tests", "allocation_dist_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        stdout, _ = p.communicate(timeout=600)
        assert p.returncode == 0, stdout.decode()[-3000:]
    res = [json.load(open(f"{out}.{r}")) for r in range(2)]
    whole = json.loads(json.dumps(_sim().compare_allocations(WM, SPLITS, DIST_PATHS, paired=True, outcomes=True)))
    for r in res:
        assert r["document"] == whole
        assert r["shard"][1] < DIST_PATHS                                        # each rank ran a part of the range only
    assert sorted(tuple(r["shard"]) for r in res) == [(0, 2502), (2502, 2501)]


def _cli(*extra):
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--seed", "7", "--working-months", str(WM), *extra]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    return r.returncode, (json.loads(r.stdout.strip().splitlines()[-1]) if r.stdout.strip() else None), r.stderr


def test_cli_allocation_table():
    rc, out, err = _cli("--paths", "2000", "--allocations", "0,0.3,0.6,1", "--paired", "--outcomes")
    assert rc == 0, err[-3000:]
    assert set(out) == {"scenario", "rng", "working_months", "num_simulations", "options", "best", "tied_with_best", "all_succeed",
                        "none_succeed", "seconds"}
    assert out["working_months"] == WM and out["num_simulations"] == 2000 and out["rng"] == "philox"
    assert [r["allocation_inv1_pct"] for r in out["options"]] == [0.0, 0.3, 0.6, 1.0]
    assert all(set(r) == set(ALLOCATION_OPTION_FIELDS) | {"probability", "vs_best"} | OUTCOME_KEYS for r in out["options"])
    probs = [r["probability"] for r in out["options"]]
    assert out["best"] == probs.index(max(probs)) and out["best"] in out["tied_with_best"]
    sim = RetirementMonteCarloSimulator(Config(**dict(SCENARIOS["config"], num_simulations_main=2000)), main_seed_override=7)
    sim.use_final_seeds()
    assert probs == sim.success_probability_by_allocations(WM, [0.0, 0.3, 0.6, 1.0]).tolist()
    plain = _cli("--paths", "2000", "--allocations", "0,0.3,0.6,1")[1]
    assert [r["probability"] for r in plain["options"]] == probs and set(plain["options"][0]) == set(ALLOCATION_OPTION_FIELDS) | {"probability"}
    rc, out, _ = _cli("--paths", "2000", "--allocations", "0.2,1.5")                 # a bad split: the record builder's words, as JSON
    assert rc == 2 and "allocations[1].allocation_inv1_pct" in out["error"]


def test_cli_best_allocation():
    rc, out, err = _cli("--search-paths", "5000", "--best-allocation", "--allocation-resolution", "0.05")
    assert rc == 0, err[-3000:]
    assert set(out) == {"scenario", "rng", "working_months", "own_allocation_inv1_pct", "best_allocation_inv1_pct", "probability", "tied",
                        "probes", "curve", "seconds"}
    assert out["own_allocation_inv1_pct"] == 0.6 and out["probes"] == 2               # 0.1 -> 0.05: the grid and one refinement
    points = [c["allocation_inv1_pct"] for c in out["curve"]]
    assert points[:11] == [i / 10.0 for i in range(11)] and len(points) in (12, 13) and set(out["curve"][0]) == {"allocation_inv1_pct", "probability"}
    sim = RetirementMonteCarloSimulator(Config(**dict(SCENARIOS["config"], num_simulations_search=5000)), main_seed_override=7)
    got = sim.find_best_allocation(WM, resolution=0.05, verbose=False)
    assert (out["best_allocation_inv1_pct"], out["probability"], out["curve"], out["tied"]) == got
    assert out["best_allocation_inv1_pct"] in out["tied"]
