"""Yearly bins under a spending rule (`mcr_run_rule_year_bins_rng`, path_kernel's MODE 3 with RULE) on the GPU: held to the plain
yearly-bins launch under the neutral rule, to `mcr_run_rule_rng`'s own rows, counts and summary under rules that fire, and through
those rows to the unmodified CPU oracle (tests/spending_rule_model.py).

600 paths of `spending_rule_model.plan_config` plans (30 retirement years): three 256-thread workgroups, the last ragged, with a
ragged last wave; one 5 003-path case for several workgroups per CU.  Seed, stream and expense levels are the spending-rule
tests' (`spending_rule_model.SEED` / `STREAM` / `LEVELS`): 10-90 % of the paths fail and cuts, floors and raises all occur."""

from __future__ import annotations

import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import bin_rule
import spending_rule_model as M
from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd import results as R
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
from monte_carlo_retirement_amd.spending_rules import SpendingBands, SpendingRule
from test_gpu_spending_rule import MONTHS, N_PATHS, PLANS, _params, _rule, _summary_launch   # the rule launch's rows: run once, shared
from test_gpu_year_bins import BLOCKS, TABLES, _cells

pytestmark = pytest.mark.gpu
SEED, STREAM = M.SEED, M.STREAM
RY = 30
EDGES, WR_EDGES = E.default_year_edges(64), E.default_wr_edges(64)
M_EDGES = np.linspace(0.5, 1.5, 65)
RULE_BLOCKS = ("rule_year_counts", "multiplier_bins")
_counts = {}


def _bins(p, wm, rule, n=N_PATHS, begin=0, edges=EDGES, wr_edges=WR_EDGES, m_edges=M_EDGES, into=None):
    return E.run_rule_year_bins_host(p, SEED, STREAM, begin, n, wm, rule, edges=edges, wr_edges=wr_edges, m_edges=m_edges, into=into)


def _count_launch(plan, wm, rname):
    """counters, year_counts, wr_obs_counts and ruin_year_bins of the count-only `mcr_run_rule_rng` launch of one case, run once."""
    import torch

    key = (plan, wm, rname)
    if key not in _counts:
        p = _params(plan, wm, rname)
        sz = E.query_sizes(p, wm)
        dev = torch.device("cuda", 0)
        wr_obs = torch.zeros(sz.retirement_years, dtype=torch.int64, device=dev)
        ruin = torch.zeros(sz.ruin_bins, dtype=torch.int64, device=dev)
        res = E.run_rule(p, SEED, STREAM, 0, N_PATHS, wm, _rule(rname), out_extra={"wr_obs_counts": wr_obs.data_ptr(), "ruin_year_bins": ruin.data_ptr()})
        counts = res["counts"].cpu().numpy()
        _counts[key] = {"counters": counts[:2].astype(np.uint64), "year_counts": counts[2:].reshape(-1, 4).astype(np.uint64),
                        "wr_obs_counts": wr_obs.cpu().numpy().astype(np.uint64), "ruin_year_bins": ruin.cpu().numpy().astype(np.uint64)}
    return _counts[key]


def _row_start(wm):
    return wm // 12 + (1 if wm % 12 else 0)         # the sample at retirement: row num_working_years


def _check_against_rule_launch(yb, rows, summ, cnt, n, wm):
    """One launch's tables against the rows, summary and counts of `mcr_run_rule_rng` over the same paths (test 2 of the issue)."""
    for k in ("counters", "wr_obs_counts", "ruin_year_bins"):
        assert yb[k].tolist() == cnt[k].tolist(), k
    assert np.array_equal(yb["rule_year_counts"], cnt["year_counts"])
    me = yb["m_edges"]
    exp_m = np.stack([_cells(r, me) for r in rows])
    assert np.array_equal(yb["multiplier_bins"].astype(np.int64), exp_m)
    ok = summ["success"].astype(bool)
    assert np.array_equal(yb["final_success_bins"].astype(np.int64), _cells(summ["final_balance"][ok], yb["edges"]))
    assert np.array_equal(yb["trajectory_bins"][_row_start(wm)].astype(np.int64), _cells(summ["start_balance"], yb["edges"]))
    assert np.all(yb["trajectory_bins"].sum(axis=1) == n) and np.all(yb["real_trajectory_bins"].sum(axis=1) == n)
    assert np.array_equal(yb["wr_bins"].sum(axis=1), yb["wr_obs_counts"])
    assert np.array_equal(yb["multiplier_bins"].sum(axis=1), yb["rule_year_counts"][:, N.MCR_RULE_ALIVE])
    assert int(yb["final_success_bins"].sum()) == int(yb["counters"][0]) == int(ok.sum())


# ---- 1. the neutral rule is the plain yearly-bins launch --------------------------------------------------------------------
@pytest.mark.parametrize("wm", MONTHS)
@pytest.mark.parametrize("plan", PLANS)
def test_neutral_rule_equals_plain_year_bins(plan, wm):
    p = _params(plan, wm, "neutral")
    plain = E.run_year_bins_host(p, SEED, STREAM, 0, N_PATHS, wm, edges=EDGES, wr_edges=WR_EDGES)
    got = _bins(p, wm, _rule("neutral"))
    for k in BLOCKS:
        assert np.array_equal(got[k], plain[k]), (plan, wm, k)
    one = int(np.argmax(_cells(np.array([1.0]), M_EDGES)))
    alive = got["rule_year_counts"][:, N.MCR_RULE_ALIVE]
    assert np.array_equal(got["multiplier_bins"][:, one], alive) and int(got["multiplier_bins"].sum()) == int(alive.sum())
    assert np.all(got["rule_year_counts"][:, 1:] == 0) and int(alive[0]) > 0
    assert 0.10 * N_PATHS <= N_PATHS - int(got["counters"][0]) <= 0.90 * N_PATHS
    # the default edges of the neutral rule are one point, 64 zero-width bins: legal, and 1.0 lands in the last of them
    z = E.run_rule_year_bins_host(p, SEED, STREAM, 0, N_PATHS, wm, _rule("neutral"), edges=EDGES, wr_edges=WR_EDGES)
    assert z["m_edges"].tolist() == [1.0] * 65 and np.array_equal(z["multiplier_bins"][:, 64], alive)
    for k in BLOCKS:
        assert np.array_equal(z[k], plain[k]), (plan, wm, k)


# ---- 2. the rule's outputs are mcr_run_rule_rng's -----------------------------------------------------------------------------
@pytest.mark.parametrize("rname", ("cut_only", "symmetric"))
@pytest.mark.parametrize("wm", MONTHS)
@pytest.mark.parametrize("plan", PLANS)
def test_rule_outputs_equal_the_rule_launch(plan, wm, rname):
    p = _params(plan, wm, rname)
    summ = _summary_launch(plan, wm, rname)
    yb = _bins(p, wm, _rule(rname))
    _check_against_rule_launch(yb, summ["multipliers"], summ, _count_launch(plan, wm, rname), N_PATHS, wm)
    yc = yb["rule_year_counts"].astype(np.int64)
    assert yc[:, N.MCR_RULE_CUT].sum() > 0 and yc[:, N.MCR_RULE_FLOOR].sum() > 0
    assert (yc[:, N.MCR_RULE_RAISED].sum() > 0) == (rname == "symmetric")


def test_several_workgroups_per_cu():
    """5 003 paths (20 workgroups, ragged): the tables against the rule launch's own rows of the same paths."""
    plan, wm, rname, n = "streams", 7, "symmetric", 5003
    p, rule = _params(plan, wm, rname), _rule(rname)
    summ = E.run_rule_host(p, SEED, STREAM, 0, n, wm, rule, want="summary", multipliers=True)
    yb = _bins(p, wm, rule, n=n)
    me = yb["m_edges"]
    assert np.array_equal(yb["multiplier_bins"].astype(np.int64), np.stack([_cells(r, me) for r in summ["multipliers"]]))
    assert np.array_equal(yb["rule_year_counts"], summ["year_counts"]) and yb["counters"].tolist() == summ["counters"].tolist()
    ok = summ["success"].astype(bool)
    assert np.array_equal(yb["final_success_bins"].astype(np.int64), _cells(summ["final_balance"][ok], EDGES))
    assert np.array_equal(yb["trajectory_bins"][_row_start(wm)].astype(np.int64), _cells(summ["start_balance"], EDGES))
    assert np.all(yb["trajectory_bins"].sum(axis=1) == n) and np.array_equal(yb["wr_bins"].sum(axis=1), yb["wr_obs_counts"])


# ---- 3. edge sets, and any subset of tables ----------------------------------------------------------------------------------
def _raw_call(p, wm, rule, edges, wr_edges, m_edges, skip=(), n=N_PATHS):
    """The host entry point with any subset of the tables NULL; returns the tables it was given (zeroed before)."""
    sz = E.query_sizes(p, wm)
    T, ry = sz.trajectory_len, sz.retirement_years
    e, we, me = (np.ascontiguousarray(x, dtype=np.float64) for x in (edges, wr_edges, m_edges))
    nb, nw, nm = e.size - 1, we.size - 1, me.size - 1
    res = {"counters": np.zeros(2, np.uint64), "wr_obs_counts": np.zeros(ry, np.uint64), "ruin_year_bins": np.zeros(sz.ruin_bins, np.uint64),
           "trajectory_bins": np.zeros((T, nb + 2), np.uint64), "real_trajectory_bins": np.zeros((T, nb + 2), np.uint64),
           "wr_bins": np.zeros((ry, nw + 2), np.uint64), "final_success_bins": np.zeros(nb + 2, np.uint64),
           "rule_year_counts": np.zeros((ry, 4), np.uint64), "multiplier_bins": np.zeros((ry, nm + 2), np.uint64)}
    ptr = {k: (None if k in skip else v.ctypes.data) for k, v in res.items()}
    o = N.McrOutputs()
    o.counters, o.wr_obs_counts, o.ruin_year_bins = ptr["counters"], ptr["wr_obs_counts"], ptr["ruin_year_bins"]
    y = N.McrYearBins()
    y.edges, y.n_bins, y.wr_edges, y.n_wr_bins = e.ctypes.data, nb, we.ctypes.data, nw
    for k in TABLES:
        setattr(y, k, ptr[k])
    r = N.McrRuleYearBins()
    r.m_edges, r.n_m_bins, r.multiplier_bins, r.year_counts = me.ctypes.data, nm, ptr["multiplier_bins"], ptr["rule_year_counts"]
    rec, rng = rule.record(), N.philox_rng(SEED)
    rc = N.load_library().mcr_run_rule_year_bins_host_rng(C.byref(p), C.byref(rng), STREAM, 0, n, wm, C.byref(rec), C.byref(o), C.byref(y), C.byref(r), 0)
    N.check(rc, "mcr_run_rule_year_bins_host_rng")
    return res


def test_multiplier_edge_sets_and_null_tables():
    plan, wm, rname = "streams", 7, "symmetric"
    p, rule = _params(plan, wm, rname), _rule(rname)
    summ, cnt = _summary_launch(plan, wm, rname), _count_launch(plan, wm, rname)
    rows = summ["multipliers"]
    floor, ceiling = M.RULES[rname][4], M.RULES[rname][5]
    vals = rows[~np.isnan(rows)]
    assert vals.min() == floor and np.any(vals == 1.0) and floor < vals.max() <= ceiling    # the multiplier sits exactly on those values
    sets = {
        "one_bin": np.array([floor, ceiling]),
        "zero_width": np.array([0.5, 0.5, 0.81, 0.81, 0.81, 1.0, 1.0, 1.5]),
        "on_the_values": np.array([0.0, floor, 0.9, 1.0, 1.1, ceiling, 2.0]),
        "floor_one_ceiling_only": np.array([floor, 1.0, ceiling]),
        "all_above": np.array([0.0, 0.1, 0.2]),
        "all_below": np.array([2.0, 3.0, 4.0]),
    }
    for name, me in sets.items():
        yb = _bins(p, wm, rule, m_edges=me)
        _check_against_rule_launch(yb, rows, summ, cnt, N_PATHS, wm)
        if name == "all_above":
            assert np.array_equal(yb["multiplier_bins"][:, -1], cnt["year_counts"][:, 0])
        if name == "all_below":
            assert np.array_equal(yb["multiplier_bins"][:, 0], cnt["year_counts"][:, 0])
    # 512 + 512 + 512 bins, the LDS cap (on a plan without a frozen stream: its column would not fit beside them)
    plan = "realized"
    p2 = _params(plan, wm, rname)
    top = float(_summary_launch(plan, wm, rname)["final_balance"].max())
    big = _bins(p2, wm, rule, edges=E.default_year_edges(N.MCR_MAX_YEAR_BINS, hi=max(top * 4.0, 1e7)),
                wr_edges=E.default_wr_edges(N.MCR_MAX_YEAR_BINS, 50.0), m_edges=np.linspace(0.5, 1.5, N.MCR_MAX_YEAR_BINS + 1))
    assert big["multiplier_bins"].shape == (RY, 514) and big["trajectory_bins"].shape[1] == 514 and big["wr_bins"].shape[1] == 514
    _check_against_rule_launch(big, _summary_launch(plan, wm, rname)["multipliers"], _summary_launch(plan, wm, rname), _count_launch(plan, wm, rname), N_PATHS, wm)
    # any subset of the tables NULL: the others are what they are with all of them
    full = _raw_call(p, wm, rule, EDGES, WR_EDGES, M_EDGES)
    ref = _bins(p, wm, rule)
    for k in BLOCKS + RULE_BLOCKS:
        assert np.array_equal(full[k], ref[k]), k
    subsets = [("multiplier_bins",), ("rule_year_counts",), RULE_BLOCKS, TABLES, TABLES + ("multiplier_bins",), ("trajectory_bins", "wr_bins", "rule_year_counts"),
               ("counters", "wr_obs_counts", "ruin_year_bins"), ("real_trajectory_bins", "final_success_bins", "wr_obs_counts"),
               tuple(k for k in BLOCKS + RULE_BLOCKS if k != "multiplier_bins")]
    for skip in subsets:
        got = _raw_call(p, wm, rule, EDGES, WR_EDGES, M_EDGES, skip=skip)
        for k in BLOCKS + RULE_BLOCKS:
            assert np.array_equal(got[k], np.zeros_like(full[k]) if k in skip else full[k]), (skip, k)


# ---- 4. accumulation, partition, the pad loop ----------------------------------------------------------------------------------
def test_accumulation_partition_and_the_pad_loop():
    plan, wm, rname = "annual", 120, "symmetric"
    p, rule = _params(plan, wm, rname), _rule(rname)
    one = _bins(p, wm, rule)
    two = _bins(p, wm, rule, n=333)
    _bins(p, wm, rule, n=N_PATHS - 333, begin=333, into=two)
    for k in BLOCKS + RULE_BLOCKS:
        assert np.array_equal(one[k], two[k]), k
    _bins(p, wm, rule, into=two)                               # `into` accumulates
    for k in BLOCKS + RULE_BLOCKS:
        assert np.array_equal(two[k], 2 * one[k]), k
    with pytest.raises(ValueError):
        _bins(p, wm, rule, m_edges=np.linspace(0.5, 1.5, 9), into=two)
    b = E.YearBinsBatch(p, wm, EDGES, WR_EDGES, rule=rule, m_edges=M_EDGES)        # the device-resident batch: two launches, one vector
    b.launch(SEED, STREAM, 0, 333)
    b.launch(SEED, STREAM, 333, N_PATHS - 333)
    host = b.host()
    at = b.reduce_vec.data_ptr()
    for k in BLOCKS + RULE_BLOCKS:
        assert np.array_equal(host[k].astype(np.uint64), one[k]), k
        v = getattr(b, k)
        assert v.data_ptr() == at and v.is_contiguous()
        at += v.numel() * 8
    assert at == b.reduce_vec.data_ptr() + b.reduce_vec.numel() * 8
    # a mostly-failing plan: whole waves are dead long before the last year and pad their rows
    cfg = dict(M.plan_config(plan, REPO, wm), monthly_expenses=3.0 * M.LEVELS[plan, wm][rname])
    hard = params_from_config(Config(**cfg))
    summ = E.run_rule_host(hard, SEED, STREAM, 0, N_PATHS, wm, rule, want="summary", multipliers=True)
    rows = summ["multipliers"]
    dead = np.isnan(rows).all(axis=1)
    assert dead[-1] and not dead[0] and int(summ["counters"][0]) < 0.1 * N_PATHS
    first_dead = int(np.argmax(dead))
    yb = _bins(hard, wm, rule)
    assert not yb["multiplier_bins"][first_dead:].any() and not yb["rule_year_counts"][first_dead:].any()
    assert np.array_equal(yb["multiplier_bins"].astype(np.int64), np.stack([_cells(r, M_EDGES) for r in rows]))
    zero = int(np.argmax(_cells(np.array([0.0]), EDGES)))
    T = yb["trajectory_bins"].shape[0]
    for t in range(T - RY + first_dead, T):                   # every path is dead in these years: exact zeros, nominal and real
        assert int(yb["trajectory_bins"][t, zero]) == N_PATHS and int(yb["real_trajectory_bins"][t, zero]) == N_PATHS
    assert np.array_equal(yb["rule_year_counts"], summ["year_counts"]) and yb["counters"].tolist() == summ["counters"].tolist()


# ---- 5. what the entry point refuses ---------------------------------------------------------------------------------------------
def test_unsupported_requests_are_refused_by_name_and_compute_nothing():
    from test_rule_year_bins_cpu import Call

    call = Call(N.load_library())
    rc, msg, untouched = call.run()
    assert rc == 0 and not untouched, (rc, msg)                 # the request itself is a valid one
    history = N.history_rng(SEED, np.random.default_rng(1).standard_normal((240, 3)), 12)
    many = dict(M.plan_config("realized", REPO, 7))
    many["other_income_streams"] = [{"name": f"s{k}", "monthly_amount_today": 100.0 + k, "start_at_age": 50.0 + k, "duration_years": None,
                                     "inflation_indexed": True, "tax_rate": 0.1} for k in range(17)]
    p17 = params_from_config(Config(**many))
    for what, kw, code, word in [("the history stream", dict(rng=history), N.MCR_ERR_UNSUPPORTED, "history stream"),
                                 ("the NumPy stream", dict(rng=N.numpy_rng(12345)), N.MCR_ERR_UNSUPPORTED, "NumPy stream"),
                                 ("a 17-stream block", dict(params=p17), N.MCR_ERR_UNSUPPORTED, "17 income streams"),
                                 ("the in-kernel histogram", dict(hist=True), N.MCR_ERR_UNSUPPORTED, "hist_bins"),
                                 ("a per-path pointer", dict(per_path=True), N.MCR_ERR_INVALID_ARG, "per-path")]:
        rc, msg, untouched = call.run(**kw)
        assert rc == code and word in msg and untouched, (what, rc, msg, untouched)
    with pytest.raises(RuntimeError, match="code -4"):
        E.run_rule_year_bins_host(p17, SEED, STREAM, 0, N_PATHS, 7, _rule("cut_only"))


# ---- 6. two ranks, one all-reduce --------------------------------------------------------------------------------------------------
def test_two_ranks_one_all_reduce(tmp_path):
    from rule_year_bins_dist_worker import N_PATHS as N_DIST, PLAN, RNAME, WM

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res")
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                       os.path.join(REPO, "tests", "rule_year_bins_dist_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for pr in procs:
        stdout, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, stdout.decode()[-3000:]
    whole = _bins(_params(PLAN, WM, RNAME), WM, _rule(RNAME), n=N_DIST)
    vec = np.concatenate([whole[k].reshape(-1) for k in BLOCKS + RULE_BLOCKS]).astype(np.int64)
    shards = []
    for rank in range(2):
        r = json.load(open(f"{out}.{rank}"))
        assert r["vector"] == vec.tolist(), rank
        assert r["exchange"] == f"1 all-reduce(sum) of {vec.size} int64 words" and r["collectives"] == 1
        assert r["m_edges"] == M_EDGES.tolist()
        shards.append(tuple(r["shard"]))
    assert sorted(shards) == [(0, N_DIST - N_DIST // 2), (N_DIST - N_DIST // 2, N_DIST // 2)]


# ---- 7. the document and the command line ---------------------------------------------------------------------------------------
def _simulator(plan, wm, rname, n):
    cfg = Config(**dict(M.plan_config(plan, REPO, wm), monthly_expenses=M.LEVELS[plan, wm][rname], num_simulations_main=n, seed=11))
    sim = RetirementMonteCarloSimulator(cfg, main_seed_override=2024)
    sim.use_final_seeds()
    return cfg, sim


def test_streamed_document_under_a_rule():
    plan, wm, rname, n = "streams", 120, "symmetric", 3000
    rule = _rule(rname)
    cfg, sim = _simulator(plan, wm, rname, n)
    doc = json.loads(json.dumps(R.streamed_result(cfg, sim, wm, rule=rule)))
    assert doc["spending_rule"] == rule.as_dict()
    assert {"trajectory.samples", "trajectory_real.samples", "summary.swr"} <= set(doc["not_available"])
    assert doc["trajectory"]["sample_paths"] is None and doc["trajectory_real"]["sample_paths"] is None
    sp, br = doc["spending"], doc["band_brackets"]["spending"]
    assert sp["base_monthly_expenses"] == cfg.monthly_expenses and len(sp["years"]) == RY
    assert set(sp["percentiles"]) == {"p5", "p25", "p50", "p75", "p95"} == set(br["lo"]) == set(br["hi"])
    for key, est in sp["percentiles"].items():
        assert len(est) == RY
        for lo, v, hi in zip(br["lo"][key], est, br["hi"][key]):
            assert lo is not None and hi is not None and lo <= v <= hi, (key, lo, v, hi)
    # the exact median of the rule launch's own multiplier rows x the base expenses lies inside its bracket, every year
    params, rng = sim._current_params(), sim._batch_rng(n)
    ref = E.run_rule_host(params, rng, sim._stream_id, 0, n, wm, rule, multipliers=True)
    for y in range(RY):
        row = ref["multipliers"][y]
        exact = round(float(np.median(row[~np.isnan(row)]) * cfg.monthly_expenses), 2)       # (the brackets are rounded to cents: monotone)
        assert br["lo"]["p50"][y] <= exact <= br["hi"]["p50"][y], (y, br["lo"]["p50"][y], exact, br["hi"]["p50"][y])
    # the shares are the year counts, exactly
    yc = ref["year_counts"].astype(np.float64)
    for y, row in enumerate(sp["years"]):
        assert [row["alive"], row["cut"], row["at_floor"], row["raised"]] == (yc[y] / n).tolist(), y
    assert doc["summary"]["success_probability"] == float(np.float64(int(ref["counters"][0])) / np.float64(n) * 100.0)
    # sim.spending_rule_fan_chart: the same tables and bands
    _, sim_b = _simulator(plan, wm, rname, n)
    fan = sim_b.spending_rule_fan_chart(wm, rule)
    assert np.array_equal(fan["rule_year_counts"].astype(np.uint64), ref["year_counts"]) and fan["outcomes"].successes == int(ref["counters"][0])
    assert isinstance(fan["spending"], SpendingBands) and [round(float(v), 2) for v in fan["spending"].estimate[:, 2]] == sp["percentiles"]["p50"]
    # under the neutral rule every key shared with the plain streamed document is equal, except the samples
    cfg_n, sim_n = _simulator(plan, wm, "neutral", n)
    ruled = json.loads(json.dumps(R.streamed_result(cfg_n, sim_n, wm, rule=SpendingRule.neutral())))
    _, sim_p = _simulator(plan, wm, "neutral", n)
    plain = json.loads(json.dumps(R.streamed_result(cfg_n, sim_p, wm)))
    assert set(plain) <= set(ruled) and set(ruled) - set(plain) == {"spending_rule", "spending"}
    for k in plain:
        a, b = ruled[k], plain[k]
        if k in ("trajectory", "trajectory_real"):
            a, b = ({x: v for x, v in d.items() if x != "sample_paths"} for d in (a, b))
            assert len(plain[k]["sample_paths"]) == 5
        elif k == "not_available":
            a = [x for x in a if not x.endswith(".samples")]
        elif k == "band_brackets":
            a = {x: v for x, v in a.items() if x != "spending"}
        assert a == b, k


def test_cli_spending_rule_streamed(tmp_path):
    cfg = dict(M.plan_config("streams", REPO, 120), monthly_expenses=M.LEVELS["streams", 120]["symmetric"], num_simulations_main=3000, seed=11)
    path = tmp_path / "scenario.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "run_scenario.py"), str(path), "--working-months", "120",
                          "--spending-rule", ",".join(str(x) for x in M.RULES["symmetric"]), "--streamed"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    doc = json.loads(out.stdout[out.stdout.index("{"):])
    assert doc["spending_rule"] == SpendingRule(*M.RULES["symmetric"]).as_dict() and len(doc["spending"]["years"]) == RY
    assert "trajectory.samples" in doc["not_available"] and "spending" in doc["band_brackets"]
    assert doc["histogram_binned"]["total_paths"] == 3000 and len(doc["trajectory"]["percentiles"]["p50"]) == len(doc["trajectory"]["years"])


# ---- 8. rules that fire, against the reference arithmetic ----------------------------------------------------------------------
@pytest.mark.parametrize("rname", ("cut_only", "symmetric"))
@pytest.mark.parametrize("wm", MONTHS)
@pytest.mark.parametrize("plan", PLANS)
def test_firing_rules_vs_the_oracle(oracle, plan, wm, rname):
    """Every path's OWN multiplier row (mcr_run_rule_rng's; test_rule_outputs_equal_the_rule_launch ties it to this launch) is a
    deterministic expense schedule the unmodified oracle can run (`spending_rule_model.run_path`): its trajectory, real trajectory,
    withdrawal rates and successful final balances, binned on the launch's edges, against the launch's tables.  The comparison is
    test_gpu_year_bins.test_tables_vs_oracle's, statement for statement: a row that is not exactly equal may move at most
    2 x (its entries within 1e-8 relative of an edge); the counters are equal exactly.  (The schedule's arithmetic, E max(m) minus a
    stream, differs from (E m) price by roundings `spending_rule_model.verify` bounds with the differential test's ABS / REL.)

    Measured on an MI355X (600 paths a case, all 18 cases): counters equal, 0 entries moved, 0 entries within 1e-8 of an edge —
    every row of all four tables exactly equal (LABNOTES R29).  The figures are printed per case."""
    p = _params(plan, wm, rname)
    summ = _summary_launch(plan, wm, rname)
    rows = summ["multipliers"]
    cols = {"trajectory": [], "real_trajectory": [], "withdrawal_rate_trajectory": [], "final_balance": [], "success": []}
    for i in range(N_PATHS):
        sched, last = [], 1.0
        for y in range(RY):                          # years the path does not begin: the last multiplier it had (as `verify` runs it)
            if not np.isnan(rows[y, i]):
                last = float(rows[y, i])
            sched.append(last)
        run = M.run_path(p, wm, SEED, STREAM, i, sched)
        for k in ("trajectory", "real_trajectory", "withdrawal_rate_trajectory"):
            cols[k].append(run[k][:, 0])
        cols["final_balance"].append(float(run["final_balance"][0]))
        cols["success"].append(bool(run["success"][0]))
    c = {k: np.stack(v, axis=1) for k, v in cols.items() if k.endswith("trajectory")}
    ok = np.array(cols["success"])
    fin = np.array(cols["final_balance"])
    yb = _bins(p, wm, _rule(rname))
    assert yb["counters"].tolist() == [int(ok.sum()), N_PATHS]
    data_rows = [("trajectory_bins", c["trajectory"], yb["edges"]), ("real_trajectory_bins", c["real_trajectory"], yb["edges"]),
                 ("wr_bins", c["withdrawal_rate_trajectory"], yb["wr_edges"]), ("final_success_bins", fin[ok][None, :], yb["edges"])]
    moved_total = near_total = 0
    failures = []
    for name, data, edges in data_rows:
        got = yb[name].astype(np.int64).reshape(data.shape[0], -1)
        for t, row in enumerate(data):
            moved, near, wrong = bin_rule.row_verdict(got[t], row, edges)      # (the edge at 0 apart: tests/bin_rule.py)
            moved_total, near_total = moved_total + moved, near_total + near
            if wrong is not None:
                failures.append(f"{name}[{t}]: {wrong}")
    print(f"{plan} wm={wm} {rname}: entries moved {moved_total}, entries within 1e-8 of an edge {near_total}, rows over the bound {len(failures)}")
    assert not failures, failures
