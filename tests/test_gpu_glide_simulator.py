"""The glide-path methods of `RetirementMonteCarloSimulator` on the GPU: `success_probability_by_glide_paths` and
`compare_glide_paths` (the catalogue and an explicit list, with and without the paired and outcome keys) against `engine` rows
and against the allocation methods for constant tables, two ranks on one card against the single process, and the
command-line tool."""

from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from glide_dist_worker import N_PATHS as DIST_PATHS, OPTIONS, WM, make_simulator as _sim
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.allocation import SCENARIO_FIELDS, GlidePath, default_glide_paths, glide_records

pytestmark = pytest.mark.gpu
DIFFERENCE_KEYS = {"delta", "se", "se_unpaired", "p_value", "rescued"}
OUTCOME_KEYS = {"lasts_until_age", "median_ruin_age", "final_balance"}
ROW_KEYS = {"name", "weights", "probability"} | set(SCENARIO_FIELDS)


def _engine_percent(sim, options, n):
    """The success % of `options` from `engine.probe_glide_paths` on the simulator's own stream."""
    records, table = glide_records(sim.params_model, options)
    engine_options = [(*r[:3], tuple(table[r[3]:r[3] + r[4]])) for r in records]
    counts = E.probe_glide_paths(sim._current_params(), sim._batch_rng(n), sim._stream_id, 0, n, WM, engine_options).cpu().numpy()
    assert N.load_library().mcr_probe_glide_paths_last_fanout_launches() == 1
    return [sim._count_percent(c[N.MCR_CTR_SUCCESS], n) for c in counts]


def test_probabilities_equal_engine_rows_and_the_allocation_methods():
    sim, n = _sim(), 3000
    got = sim.success_probability_by_glide_paths(WM, OPTIONS, n)
    assert got.dtype == np.float64 and got.shape == (len(OPTIONS),)
    assert got.tolist() == _engine_percent(sim, OPTIONS, n)
    assert got[0] == got[1] == sim.success_probability_by_allocations(WM, [0.6], n)[0]          # a constant table is a constant split
    assert len(set(got.tolist())) >= 3                                                          # the paths do differ
    assert sim.joint_outcomes_by_glide_paths(WM, OPTIONS, n).probabilities.tobytes() == got.tobytes()
    assert sim.option_outcomes_by_glide_paths(WM, OPTIONS, n).probabilities.tobytes() == got.tobytes()
    constants = [0.0, 0.3, 0.6, 1.0]
    assert sim.success_probability_by_glide_paths(WM, [[a] * 7 for a in constants], n).tolist() == \
        sim.success_probability_by_allocations(WM, constants, n).tolist()
    assert sim.success_probability_by_glide_paths(WM, [], n).shape == (0,)
    with pytest.raises(ValueError, match=r"glide_paths\[1\]"):
        sim.success_probability_by_glide_paths(WM, [0.5, [0.2, 1.5]], n)
    with pytest.raises(ValueError, match="inv1_returns_mean"):
        sim.success_probability_by_glide_paths(WM, [{"glide_path": 0.5, "inv1_returns_mean": 0.1}], n)
    numpy_sim = _sim(rng="numpy")
    with pytest.raises(RuntimeError, match="NumPy stream is not supported under a glide path"):
        numpy_sim.success_probability_by_glide_paths(WM, [0.5, [0.9, 0.1]], n)


def test_compare_documents_extend_the_plain_one():
    sim, n = _sim(), 3000
    plain = sim.compare_glide_paths(WM, OPTIONS, num_simulations=n)
    assert set(plain) == {"options", "best"} and len(plain["options"]) == len(OPTIONS)
    assert all(set(r) == ROW_KEYS for r in plain["options"])
    assert plain["options"][2]["weights"] == list(GlidePath.linear(0.9, 0.4, 0, 20).weights) and plain["options"][3]["weights"] == [1.0, 0.0]
    assert plain["options"][4]["name"] == "0.3>0.6@20-35" and plain["options"][5]["monthly_expenses"] == 7000.0
    assert plain["options"][0]["weights"] == plain["options"][1]["weights"] == [0.6]
    probs = [r["probability"] for r in plain["options"]]
    assert probs == sim.success_probability_by_glide_paths(WM, OPTIONS, n).tolist()
    assert plain["best"] == probs.index(max(probs))                              # the first of equals
    both = sim.compare_glide_paths(WM, OPTIONS, paired=True, outcomes=True, num_simulations=n)
    assert set(both) == set(plain) | {"tied_with_best", "all_succeed", "none_succeed"}
    added = OUTCOME_KEYS | {"vs_best"}
    stripped = dict({k: v for k, v in both.items() if k in plain}, options=[{k: v for k, v in r.items() if k not in added} for r in both["options"]])
    assert stripped == plain
    assert all(set(r) == ROW_KEYS | added for r in both["options"])
    best = both["best"]
    assert both["options"][best]["vs_best"]["delta"] == 0.0 and best in both["tied_with_best"]
    for r in both["options"]:
        assert set(r["vs_best"]) == DIFFERENCE_KEYS and r["vs_best"]["delta"] >= 0.0
        assert set(r["lasts_until_age"]) == {"90", "95", "99"} and set(r["final_balance"]) == {"p5", "p25", "p50", "p75", "p95"}
    assert both["options"][0]["vs_best"] == both["options"][1]["vs_best"]        # the duplicate
    paired = sim.compare_glide_paths(WM, OPTIONS, paired=True, num_simulations=n)
    assert dict(both, options=[{k: v for k, v in r.items() if k not in OUTCOME_KEYS} for r in both["options"]]) == paired
    # the default: the catalogue built for WM
    catalogue = default_glide_paths(sim.params_model, WM)
    default = sim.compare_glide_paths(WM, num_simulations=n)
    assert [r["name"] for r in default["options"]] == [g.describe() for g in catalogue] and len(catalogue) == 6
    assert [r["weights"] for r in default["options"]] == [list(g.weights) for g in catalogue]
    assert default["options"][0]["weights"] == [0.6] and default["options"][1]["weights"] == [1.0] and default["options"][2]["weights"] == [0.0]
    assert [r["probability"] for r in default["options"]] == _engine_percent(sim, catalogue, n)
    assert [r["probability"] for r in default["options"][:3]] == sim.success_probability_by_allocations(WM, [0.6, 1.0, 0.0], n).tolist()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_return_the_single_process_document(tmp_path):
    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    try:
        for rank in range(2):
            env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                       OMP_NUM_THREADS="1")
            procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                           os.path.join(REPO, "tests", "glide_dist_worker.py"), out], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        for p in procs:
            stdout, _ = p.communicate(timeout=300)
            assert p.returncode == 0, stdout.decode()[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    res = [json.load(open(f"{out}.{r}")) for r in range(2)]
    whole = json.loads(json.dumps(_sim().compare_glide_paths(WM, OPTIONS, paired=True, outcomes=True, num_simulations=DIST_PATHS)))
    for r in res:
        assert r["document"] == whole
        assert r["shard"][1] < DIST_PATHS                                        # each rank ran a part of the range only
    assert sorted(tuple(r["shard"]) for r in res) == [(0, 2502), (2502, 2501)]


def _cli(*extra):
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--seed", "7", "--working-months", str(WM), *extra]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    return r.returncode, (json.loads(r.stdout.strip().splitlines()[-1]) if r.stdout.strip() else None), r.stderr


def test_cli_glide_table():
    from monte_carlo_retirement_amd import Config
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
    from test_gpu_expense_probe import SCENARIOS

    spec = "0.9>0.4@0-20;0.6;0.3>0.6@20-35"
    rc, out, err = _cli("--paths", "2000", "--glide-paths", spec, "--paired", "--outcomes")
    assert rc == 0, err[-3000:]
    assert set(out) == {"scenario", "rng", "working_months", "num_simulations", "options", "best", "tied_with_best", "all_succeed",
                        "none_succeed", "seconds"}
    assert out["working_months"] == WM and out["num_simulations"] == 2000 and out["rng"] == "philox"
    assert [r["name"] for r in out["options"]] == spec.split(";")
    assert all(set(r) == ROW_KEYS | {"vs_best"} | OUTCOME_KEYS for r in out["options"])
    assert out["options"][1]["weights"] == [0.6] and len(out["options"][0]["weights"]) == 21
    sim = RetirementMonteCarloSimulator(Config(**dict(SCENARIOS["config"], num_simulations_main=2000)), main_seed_override=7)
    sim.use_final_seeds()
    assert [r["probability"] for r in out["options"]] == sim.success_probability_by_glide_paths(WM, spec.split(";")).tolist()
    rc, out, err = _cli("--paths", "2000", "--glide-paths", "0.9>0.4@20")           # malformed: refused before any device work
    assert rc == 2 and "start>end@from-to" in (err + json.dumps(out))
