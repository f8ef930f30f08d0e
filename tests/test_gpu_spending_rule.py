"""The spending-rule launch (`mcr_run_rule_rng`, path_kernel's RULE) on the GPU, held to the plain launch under the neutral rule
and to the unmodified CPU oracle under rules that fire (tests/spending_rule_model.py).

600 paths (three workgroups, the last partial, a partial wave), 30 retirement years, working_months in {0, 7, 120} (7 puts
retirement between two plan-year ends: annual tax and trajectory samples fall mid-retirement-year), three plans derived from
scenarios/config.json (`spending_rule_model.plan_config`: realized-gains tax on both assets; annual gains tax; two income streams,
one frozen-nominal, starting in retirement year 5) and three rules (neutral, cut-only, symmetric).

Expense levels and seed (`spending_rule_model.LEVELS`, seed 20260, stream 1, paths 0 .. 599) were calibrated with the CPU model
alone: realized 1590 / 1850 / 6700, annual 1450 / 1680 / 5750 at 0 / 7 / 120 working months under both firing rules; streams
3300 / 3600 / 8600 under the cut-only rule and 3650 / 3950 / 8600 under the symmetric one; under the neutral rule 0.7 of the
cut-only level, about where half the paths of the fixed-spending plan fail.
"""

from __future__ import annotations

import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import spending_rule_model as M
from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.spending_rules import SpendingRule

pytestmark = pytest.mark.gpu
N_PATHS = 600
PLANS = ("realized", "annual", "streams")
MONTHS = (0, 7, 120)
SEED, STREAM = M.SEED, M.STREAM
_cache = {}


def _params(plan, wm, rname):
    level = M.LEVELS[plan, wm][rname]
    return params_from_config(Config(**dict(M.plan_config(plan, REPO, wm), monthly_expenses=level)))


def _rule(rname):
    return SpendingRule(*M.RULES[rname])


def _summary_launch(plan, wm, rname):
    """The summary launch with multiplier rows of one case, run once and shared."""
    key = (plan, wm, rname)
    if key not in _cache:
        _cache[key] = E.run_rule_host(_params(plan, wm, rname), SEED, STREAM, 0, N_PATHS, wm, _rule(rname), want="summary", multipliers=True)
    return _cache[key]


@pytest.mark.parametrize("wm", MONTHS)
@pytest.mark.parametrize("plan", PLANS)
def test_neutral_rule_is_the_plain_launch_bit_for_bit(plan, wm):
    p = _params(plan, wm, "neutral")
    got = _summary_launch(plan, wm, "neutral")
    ref = E.run_batch_host(p, SEED, STREAM, 0, N_PATHS, wm, want_trajectories=False, want_bins=False)
    assert got["counters"].tolist() == ref["counters"].tolist() == [int(ref["success"].sum()), N_PATHS]
    for k in E.SUMMARY_FIELDS + ("success",):
        assert np.array_equal(got[k].view(np.uint64 if got[k].dtype == np.float64 else np.uint8),
                              ref[k].view(np.uint64 if ref[k].dtype == np.float64 else np.uint8)), (plan, wm, k)
    rows = got["multipliers"]
    assert rows.shape == (30, N_PATHS) and np.all((rows == 1.0) | np.isnan(rows))
    ytr = ref["years_to_ruin"]
    begins = np.array([[M.begins_year(ytr[i], y) for i in range(N_PATHS)] for y in range(30)])
    assert np.array_equal(~np.isnan(rows), begins)
    yc = got["year_counts"].astype(np.int64)
    assert np.all(yc[:, 1:] == 0) and yc[:, N.MCR_RULE_ALIVE].tolist() == begins.sum(axis=1).tolist()
    assert 0.10 * N_PATHS <= N_PATHS - int(ref["counters"][0]) <= 0.90 * N_PATHS
    # the count-only launch (no rows): the same counters and year counts
    count = E.run_rule_host(p, SEED, STREAM, 0, N_PATHS, wm, _rule("neutral"))
    assert count["counters"].tolist() == got["counters"].tolist() and np.array_equal(count["year_counts"], got["year_counts"])


@pytest.mark.parametrize("rname", ("cut_only", "symmetric"))
@pytest.mark.parametrize("wm", MONTHS)
@pytest.mark.parametrize("plan", PLANS)
def test_firing_rules_follow_the_oracle(oracle, plan, wm, rname):
    """Every path passes `verify` against the GPU's multiplier row and summary outcome; and the case is one where the rule
    matters: 10 % .. 90 % of the paths fail, at least 5 % of the begun path-years are cut, some stand at the floor, under the
    symmetric rule some are raised, and at most 1 % of the paths have an undecidable year."""
    p, rule = _params(plan, wm, rname), M.RULES[rname]
    got = _summary_launch(plan, wm, rname)
    rows = got["multipliers"]
    undecidable = 0
    for i in range(N_PATHS):
        outcome = {"success": got["success"][i], "years_to_ruin": got["years_to_ruin"][i], "final_balance": got["final_balance"][i]}
        undecidable += int(M.verify(p, wm, rule, SEED, STREAM, i, rows[:, i], outcome))
    counts = M.year_counts_of(rows, rule)
    failed = N_PATHS - int(got["counters"][N.MCR_CTR_SUCCESS])
    begun = int(counts[:, N.MCR_RULE_ALIVE].sum())
    print(f"{plan} wm={wm} {rname}: failed {failed}/{N_PATHS}, begun path-years {begun}, cut {int(counts[:, 1].sum())}, "
          f"floor {int(counts[:, 2].sum())}, raised {int(counts[:, 3].sum())}, undecidable paths {undecidable}")
    assert 0.10 * N_PATHS <= failed <= 0.90 * N_PATHS
    assert counts[:, N.MCR_RULE_CUT].sum() >= 0.05 * begun
    assert counts[:, N.MCR_RULE_FLOOR].sum() > 0
    if rname == "symmetric":
        assert counts[:, N.MCR_RULE_RAISED].sum() > 0
    else:
        assert counts[:, N.MCR_RULE_RAISED].sum() == 0
    assert undecidable <= 0.01 * N_PATHS
    assert int(got["success"].sum()) == int(got["counters"][N.MCR_CTR_SUCCESS])


@pytest.mark.parametrize("rname", ("cut_only", "symmetric"))
@pytest.mark.parametrize("wm", MONTHS)
@pytest.mark.parametrize("plan", PLANS)
def test_year_counts_are_the_rows_counts_in_both_modes(plan, wm, rname):
    got = _summary_launch(plan, wm, rname)
    assert np.array_equal(got["year_counts"].astype(np.int64), M.year_counts_of(got["multipliers"], M.RULES[rname]))
    count = E.run_rule_host(_params(plan, wm, rname), SEED, STREAM, 0, N_PATHS, wm, _rule(rname))      # MODE 0, no rows
    assert count["counters"].tolist() == got["counters"].tolist()
    assert np.array_equal(count["year_counts"], got["year_counts"])
    assert set(count) == {"counters", "year_counts"}


@pytest.mark.parametrize("plan,wm", [("realized", 7), ("annual", 120), ("streams", 0)])
def test_partition_invariance(plan, wm):
    """[0, 300) and [300, 600) give the rows of [0, 600) bit for bit, and year counts that sum to its."""
    whole = _summary_launch(plan, wm, "symmetric")
    p, rule = _params(plan, wm, "symmetric"), _rule("symmetric")
    parts = [E.run_rule_host(p, SEED, STREAM, b, 300, wm, rule, want="summary", multipliers=True) for b in (0, 300)]
    rows = np.concatenate([x["multipliers"] for x in parts], axis=1)
    assert np.array_equal(rows.view(np.uint64), whole["multipliers"].view(np.uint64))
    assert np.array_equal(parts[0]["year_counts"] + parts[1]["year_counts"], whole["year_counts"])
    assert (parts[0]["counters"] + parts[1]["counters"]).tolist() == whole["counters"].tolist()
    for k in E.SUMMARY_FIELDS:
        assert np.array_equal(np.concatenate([x[k] for x in parts]).view(np.uint64), whole[k].view(np.uint64)), k


# ---- the Python methods -------------------------------------------------------------------------------------------------------
def _simulator(**over):
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = dict(M.plan_config("streams", REPO, 120), num_simulations_search=2000, num_simulations_main=3000, target_probability=85.0,
               seed=11)
    cfg.update(over)
    return RetirementMonteCarloSimulator(Config(**cfg))


def test_probabilities_and_search_under_the_neutral_rule_equal_the_fixed_spending_ones():
    sim = _simulator()
    levels = [0.0, 4000.0, 6020.0, 9000.0, 30000.0]
    neutral, cut_only = SpendingRule.neutral(), _rule("cut_only")
    plain = sim.success_probability_by_expenses(120, levels)
    ruled = sim.success_probability_with_rule(120, neutral, levels)
    assert isinstance(ruled, np.ndarray) and ruled.view(np.uint64).tolist() == plain.view(np.uint64).tolist()
    assert 0.0 < plain[2] < 100.0
    one = sim.success_probability_with_rule(120, neutral, levels[2])
    assert isinstance(one, float) and one == plain[2]
    sim.params_model.monthly_expenses = levels[2]
    assert sim.success_probability_with_rule(120, neutral) == plain[2]
    assert np.all(sim.success_probability_with_rule(120, cut_only, levels) >= plain)
    fixed = sim.find_maximum_monthly_expenses(120, verbose=False)
    same = sim.find_maximum_initial_expenses(120, neutral, verbose=False)
    assert same == fixed and fixed[0] > 0
    more = sim.find_maximum_initial_expenses(120, cut_only, verbose=False)
    assert more[0] >= fixed[0] and more[1] >= 85.0


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_return_the_single_process_outcomes(tmp_path):
    from spending_rule_dist_worker import N_PATHS as N_DIST, RULE, WM, make_simulator, outcomes_doc

    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                       os.path.join(REPO, "tests", "spending_rule_dist_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        stdout, _ = p.communicate(timeout=600)
        assert p.returncode == 0, stdout.decode()[-3000:]
    res = [json.load(open(f"{out}.{r}")) for r in range(2)]
    sim = make_simulator()
    rule = SpendingRule(*RULE)
    plain = outcomes_doc(sim.spending_rule_outcomes(WM, rule, N_DIST))
    rows = outcomes_doc(sim.spending_rule_outcomes(WM, rule, N_DIST, multipliers=True))
    assert plain["ever_cut"] is None and 0 < rows["ever_cut"] < N_DIST and 0 < plain["successes"] < N_DIST
    assert {k: v for k, v in rows.items() if k != "ever_cut"} == {k: v for k, v in plain.items() if k != "ever_cut"}
    for r in res:
        assert r["plain"] == plain and r["rows"] == rows
    assert sorted(tuple(r["shard"]) for r in res) == [(0, 2502), (2502, 2501)]


# ---- what the entry point refuses -----------------------------------------------------------------------------------------------
def test_unsupported_requests_are_refused_by_name_and_compute_nothing():
    import torch

    wm = 7
    p = _params("realized", wm, "cut_only")
    rule = _rule("cut_only")
    lib = N.load_library()
    dev = torch.device("cuda", 0)

    def call(params, rng, extra=None):
        """A summary request with rows into sentinel-filled buffers: (rc, message, whether anything was written)."""
        counts = torch.full((2 + 4 * 30,), -7, dtype=torch.int64, device=dev)
        success = torch.full((N_PATHS,), 9, dtype=torch.uint8, device=dev)
        rows = torch.full((30, N_PATHS), -7.0, dtype=torch.float64, device=dev)
        o = N.McrOutputs()
        o.path_stride, o.counters, o.success = N_PATHS, counts.data_ptr(), success.data_ptr()
        keep = []
        for k in (extra or ()):
            keep.append(torch.full((40, N_PATHS), -7.0, dtype=torch.float64, device=dev))
            setattr(o, k, keep[-1].data_ptr())
        ro = N.McrRuleOutputs()
        ro.year_counts, ro.multipliers, ro.path_stride = counts[2:].data_ptr(), rows.data_ptr(), N_PATHS
        rec = rule.record()
        rng = E._as_rng(rng, 0)
        rc = lib.mcr_run_rule_rng(C.byref(params), C.byref(rng), STREAM, 0, N_PATHS, wm, C.byref(rec), C.byref(o), C.byref(ro), 0, None)
        torch.cuda.synchronize()
        touched = bool((counts != -7).any() or (success != 9).any() or (rows != -7.0).any() or any((t != -7.0).any() for t in keep))
        return rc, N.last_error(), touched

    rc, msg, touched = call(p, SEED)
    assert rc == 0 and touched                                       # the request itself is a valid one
    history = N.history_rng(SEED, np.random.default_rng(1).standard_normal((240, 3)), 12)
    many = dict(M.plan_config("realized", REPO, wm))
    many["other_income_streams"] = [{"name": f"s{k}", "monthly_amount_today": 100.0 + k, "start_at_age": 50.0 + k, "duration_years": None,
                                     "inflation_indexed": True, "tax_rate": 0.1} for k in range(17)]
    p17 = params_from_config(Config(**many))
    assert p17.n_streams == 17
    for what, args, word in [("the NumPy stream", (p, N.numpy_rng(12345)), "NumPy stream"),
                             ("the history stream", (p, history), "history stream"),
                             ("a 17-stream block", (p17, SEED), "17 income streams"),
                             ("a trajectory request", (p, SEED, ("trajectory",)), "trajectories"),
                             ("a withdrawal-rate trajectory request", (p, SEED, ("withdrawal_rate_trajectory",)), "trajectories")]:
        rc, msg, touched = call(*args)
        assert rc == N.MCR_ERR_UNSUPPORTED and word in msg and not touched, (what, rc, msg, touched)
    with pytest.raises(RuntimeError, match="code -4"):
        E.run_rule_host(p17, SEED, STREAM, 0, N_PATHS, wm, rule)
