"""The glide whole-path launches through the simulator, the streamed document, the N-GPU fan chart and the command-line tool:
`glide_path_fan_chart` and `streamed_result(glide_path=...)` against the plain streamed document under a constant table,
`glide_path_summary` against `success_probability_by_glide_paths`, two ranks on one card against the single process (still ONE
all-reduce of the plain vector), and `run_scenario.py --glide-path P --streamed`."""

from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import glide_run as G
import spending_rule_model as M
from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd import results as R
from monte_carlo_retirement_amd.allocation import GlidePath
from monte_carlo_retirement_amd.simulation import SUMMARY_COLUMNS, RetirementMonteCarloSimulator, allocation_by_sample, trajectory_time_points
from monte_carlo_retirement_amd.spending_rules import SpendingRule

pytestmark = pytest.mark.gpu
SEED, STREAM = M.SEED, M.STREAM
PLAN, WM, N_PATHS = "streams", 120, 3000


def _simulator(n=N_PATHS, **over):
    cfg = Config(**dict(dict(M.plan_config(PLAN, REPO, WM), monthly_expenses=M.LEVELS[PLAN, WM]["neutral"], num_simulations_main=n, seed=11), **over))
    sim = RetirementMonteCarloSimulator(cfg, main_seed_override=2024)
    sim.use_final_seeds()
    return cfg, sim


def test_streamed_document_and_fan_chart_under_a_glide_path():
    cfg, sim = _simulator()
    a, ry = float(cfg.allocation_inv1_pct), int(cfg.retirement_years)
    # a constant table gives the plain streamed document apart from the new keys and the sample paths
    glided = json.loads(json.dumps(R.streamed_result(cfg, sim, WM, glide_path=[a, a, a])))
    _, sim_p = _simulator()
    plain = json.loads(json.dumps(R.streamed_result(cfg, sim_p, WM)))
    assert set(plain) <= set(glided) and set(glided) - set(plain) == {"glide_path", "allocation_by_sample"}
    for k in plain:
        x, y = glided[k], plain[k]
        if k in ("trajectory", "trajectory_real"):
            assert x["sample_paths"] is None and len(y["sample_paths"]) == 5
            x, y = ({f: v for f, v in d.items() if f != "sample_paths"} for d in (x, y))
        elif k == "not_available":
            assert {"trajectory.samples", "trajectory_real.samples"} <= set(x)
            x = [f for f in x if not f.endswith(".samples")]
        assert x == y, k
    assert glided["glide_path"] == {"name": f"constant {a:.4g}", "weights": [a, a, a]}
    assert glided["allocation_by_sample"] == [a] * len(glided["trajectory"]["years"])
    # a table that moves: the per-sample allocation row is the table's, the tables are the engine's
    path = GlidePath.around_retirement(WM, 0.9, 0.5, 0.3, 8, 10, "target date 90 > 50 > 30")
    _, sim_g = _simulator()
    doc = json.loads(json.dumps(R.streamed_result(cfg, sim_g, WM, glide_path=path)))
    years = trajectory_time_points(WM, ry)
    assert doc["glide_path"] == {"name": "target date 90 > 50 > 30", "weights": list(path.weights)}
    assert doc["allocation_by_sample"] == allocation_by_sample(path, WM, ry) and len(doc["allocation_by_sample"]) == len(years) == len(doc["trajectory"]["years"])
    assert doc["allocation_by_sample"][0] == 0.9 and doc["allocation_by_sample"][-1] == 0.3
    _, sim_f = _simulator()
    fan = sim_f.glide_path_fan_chart(WM, path)
    ref = E.run_glide_year_bins_host(sim_f._current_params(), sim_f._batch_rng(N_PATHS), sim_f._stream_id, 0, N_PATHS, WM, path)
    for k in G.BLOCKS:
        assert np.array_equal(np.asarray(fan[k]).astype(np.uint64), ref[k]), k
    assert fan["glide_path"] == doc["glide_path"] and fan["allocation_by_sample"] == doc["allocation_by_sample"]
    assert doc["summary"]["success_probability"] == round(float(np.float64(int(ref["counters"][0])) / np.float64(N_PATHS) * 100.0), 2)
    assert doc["histogram_binned"]["success_counts"] == [int(v) for v in ref["final_success_bins"][1:-1]]
    # every way of writing one option; a rule together with a glide path is refused
    for option in ("0.9>0.4@0-20", 0.4, [0.9, 0.5], GlidePath.constant(0.4)):
        assert len(sim_f.glide_path_fan_chart(WM, option, num_simulations=300)["allocation_by_sample"]) == len(years)
    with pytest.raises(ValueError, match="spending rule together with a glide path"):
        R.streamed_result(cfg, sim_f, WM, rule=SpendingRule.neutral(), glide_path=path)
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        sim_f.glide_path_fan_chart(WM, [0.5, 1.5])
    with pytest.raises(ValueError, match="not a mapping"):
        sim_f.glide_path_summary(WM, {"glide_path": 0.5})


def test_summary_frame_under_a_glide_path():
    cfg, sim = _simulator()
    path = GlidePath.around_retirement(WM, 0.9, 0.5, 0.3, 8, 10)
    frame = sim.glide_path_summary(WM, path)
    assert list(frame.columns) == SUMMARY_COLUMNS and len(frame) == N_PATHS and frame["Success"].dtype == bool
    share = float(np.float64(int(frame["Success"].sum())) / np.float64(N_PATHS) * 100.0)
    assert share == float(sim.success_probability_by_glide_paths(WM, [path])[0])
    ref = E.run_glide_host(sim._current_params(), sim._batch_rng(N_PATHS), sim._stream_id, 0, N_PATHS, WM, path, want="summary")
    assert G.same_bits(frame["Final Balance"].to_numpy(), ref["final_balance"]) and G.same_bits(frame["YearsToRuin"].to_numpy(), ref["years_to_ruin"])
    # under the plan's own constant split the frame is the reference run's
    a = float(cfg.allocation_inv1_pct)
    const = sim.glide_path_summary(WM, a)
    _, sim_p = _simulator()
    plain = sim_p.run_monte_carlo_simulations(WM, N_PATHS)[0]
    for c in SUMMARY_COLUMNS:
        assert G.same_bits(const[c].to_numpy(), plain[c].to_numpy()), c
    assert len(sim.glide_path_summary(WM, path, num_simulations=0)) == 0


def test_two_ranks_one_all_reduce(tmp_path):
    from glide_year_bins_dist_worker import GLIDE, LEVEL, N_PATHS as N_DIST, PLAN as DIST_PLAN, WM as DIST_WM

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res")
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                       os.path.join(REPO, "tests", "glide_year_bins_dist_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for pr in procs:
        stdout, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, stdout.decode()[-3000:]
    p = params_from_config(Config(**dict(M.plan_config(DIST_PLAN, REPO, DIST_WM), monthly_expenses=M.LEVELS[DIST_PLAN, DIST_WM][LEVEL])))
    whole = E.run_glide_year_bins_host(p, SEED, STREAM, 0, N_DIST, DIST_WM, GLIDE, edges=E.default_year_edges(64), wr_edges=E.default_wr_edges(64))
    vec = np.concatenate([whole[k].reshape(-1) for k in G.BLOCKS]).astype(np.int64)
    plain_words = E.YearBinsBatch(p, DIST_WM, E.default_year_edges(64), E.default_wr_edges(64)).reduce_vec.numel()
    assert vec.size == plain_words                              # the same vector as a plain run's
    shards = []
    for rank in range(2):
        r = json.load(open(f"{out}.{rank}"))
        assert r["vector"] == vec.tolist(), rank
        assert r["exchange"] == f"1 all-reduce(sum) of {vec.size} int64 words" and r["collectives"] == 1
        shards.append(tuple(r["shard"]))
    assert sorted(shards) == [(0, N_DIST - N_DIST // 2), (N_DIST - N_DIST // 2, N_DIST // 2)]


def test_cli_glide_path_streamed(tmp_path):
    cfg = dict(M.plan_config(PLAN, REPO, WM), monthly_expenses=M.LEVELS[PLAN, WM]["neutral"], num_simulations_main=3000, seed=11)
    path = tmp_path / "scenario.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "run_scenario.py"), str(path), "--working-months", str(WM),
                          "--glide-path", "0.9>0.4@0-20", "--streamed"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    doc = json.loads(out.stdout[out.stdout.index("{"):])
    assert doc["glide_path"] == {"name": "0.9>0.4@0-20", "weights": list(GlidePath.linear(0.9, 0.4, 0, 20).weights)}
    assert len(doc["allocation_by_sample"]) == len(doc["trajectory"]["years"]) == len(doc["trajectory"]["percentiles"]["p50"])
    assert "trajectory.samples" in doc["not_available"] and doc["trajectory"]["sample_paths"] is None
    assert doc["histogram_binned"]["total_paths"] == 3000
