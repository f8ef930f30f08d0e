"""The rule-grid probe (`mcr_probe_rule_grid_rng`; path_kernel's PHASE 6 with RULE) on the GPU, held to `mcr_run_rule_rng`: one
count-only rule launch per cell at the cell's month and level.  The existing tests hold that launch to the unmodified CPU oracle
on these plans, levels and seed (tests/test_gpu_spending_rule.py); one cell per plan is held to the oracle here as well.

Plans, rules, seed and calibrated levels are `spending_rule_model`'s: the levels were fixed on the CPU so that the rules fire on
paths 0 .. 599, so the shapes that must not be vacuous include that range and say so.  Every comparison is of integers:
equality, no tolerance.
"""

from __future__ import annotations

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
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
from monte_carlo_retirement_amd.spending_rules import SpendingRule

pytestmark = pytest.mark.gpu
RY = 30
SEED, STREAM = M.SEED, M.STREAM
MONTHS = [120, 0, 7, 120, 121]             # unsorted, a repeat, month 0
PLANS = ("realized", "annual", "streams", "untaxed2")
#: (levels per row, paths, first path): two level groups; a tail wave; fewer paths than a wave; one level per row
SHAPES = [(17, 4097, 0), (4, 700, 0), (15, 63, 7), (1, 4097, 12_345)]
KNOB = "MCR_EXPENSE_FANOUT_MIN_WAVES"      # the grid probes' minimum wave count
NEVER = str(1 << 40)
_reference = {}


def _plan_dict(plan):
    """`spending_rule_model.plan_config`; "untaxed2" = "realized" with no realized-gains tax on the second asset (the kernels
    under a rule are the generic tax mask's whatever the plan's own mask is)."""
    if plan == "untaxed2":
        return dict(M.plan_config("realized", REPO), inv2_realized_gains_tax_rate=0.0)
    return M.plan_config(plan, REPO)


def _params(plan, **over):
    return params_from_config(Config(**dict(_plan_dict(plan), **over)))


def _calibrated(plan, wm, rname):
    return M.LEVELS["realized" if plan == "untaxed2" else plan, 120 if wm == 121 else wm][rname]


def _level_rows(plan, rname, n_levels, months=MONTHS):
    """Per row: the row's calibrated level, 0.0, 1e12, then a spread around the calibrated level that differs by row."""
    rows = []
    for c, wm in enumerate(months):
        cal = _calibrated(plan, wm, rname)
        row = [cal, 0.0, 1e12] + [round(cal * (0.55 + 0.06 * k + 0.013 * c), 2) for k in range(max(0, n_levels - 3))]
        rows.append(row[:n_levels])
    return rows


def _cell(plan, rname, wm, level, n, begin):
    """The count-only rule launch of one cell: `[2 + 4 ry]` integers, computed once and shared (read only)."""
    key = (plan, rname, int(wm), float(level), int(n), int(begin))
    if key not in _reference:
        got = E.run_rule(_params(plan, monthly_expenses=float(level)), SEED, STREAM, begin, n, wm, SpendingRule(*M.RULES[rname]))
        _reference[key] = got["counts"].cpu().numpy().astype(np.int64)
    return _reference[key]


def _want(plan, rname, months, rows, n, begin):
    cells = np.array([[_cell(plan, rname, wm, x, n, begin) for x in row] for wm, row in zip(months, rows)], dtype=np.int64)
    return cells[:, :, :N.MCR_N_COUNTERS], cells[:, :, N.MCR_N_COUNTERS:].reshape(len(months), len(rows[0]), RY, N.MCR_RULE_N_COUNTS)


def _launches():
    return int(N.load_library().mcr_probe_rule_grid_last_fanout_launches())


def _groups(n_levels):
    """Level groups of a shared-route call: at most one frozen stream's lock column per wave on these plans, so a launch takes
    MCR_MAX_EXPENSE_FANOUT levels."""
    return -(-n_levels // N.MCR_MAX_EXPENSE_FANOUT)


def _probe(plan, rname, months, rows, n, begin, **kw):
    counts, years = E.probe_rule_grid(_params(plan), SEED, STREAM, begin, n, months, rows, SpendingRule(*M.RULES[rname]), **kw)
    launches = _launches()
    return counts.cpu().numpy(), None if years is None else years.cpu().numpy(), launches


# ---- 1. cells equal single rule launches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "L%d_n%d_b%d" % s)
@pytest.mark.parametrize("plan", PLANS)
def test_cells_equal_single_rule_launches(plan, shape, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    n_levels, n, begin = shape
    for rname in ("symmetric", "cut_only"):
        rows = _level_rows(plan, rname, n_levels)
        want_counts, want_years = _want(plan, rname, MONTHS, rows, n, begin)
        counts, years, launches = _probe(plan, rname, MONTHS, rows, n, begin)
        assert counts.shape == (5, n_levels, 2) and years.shape == (5, n_levels, RY, 4)
        assert np.array_equal(counts, want_counts), (plan, shape, rname)
        assert np.array_equal(years, want_years), (plan, shape, rname)
        assert np.all(counts[:, :, N.MCR_CTR_PATHS] == n)
        # the shared route on every shape (the knob's default, 0, rules out no launch: the 63-path shape fans out too)
        assert launches == _groups(n_levels), (plan, shape, rname, launches)
        if begin == 0 and n >= 600:           # the calibrated range is inside: the rules fire, and some cell neither all fails nor all passes
            cal = years[:, 0]
            assert cal[:, :, N.MCR_RULE_CUT].sum() > 0 and cal[:, :, N.MCR_RULE_FLOOR].sum() > 0, (plan, shape, rname)
            if rname == "symmetric":
                assert years[:, :, :, N.MCR_RULE_RAISED].sum() > 0, (plan, shape)
            assert np.any((counts[:, 0, 0] > 0) & (counts[:, 0, 0] < n)), (plan, shape, rname, counts[:, 0, 0])
        if n_levels >= 3:
            assert np.all(counts[:, 1, 0] >= counts[:, 0, 0]) and np.all(counts[:, 2, 0] == 0)      # no spending; 1e12 a month
        # year counts not requested: the same counters
        only, none, launches = _probe(plan, rname, MONTHS, rows, n, begin, year_counts=False)
        assert none is None and np.array_equal(only, want_counts) and launches == _groups(n_levels)


# ---- 2. the neutral rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
def test_neutral_rule_counts_what_the_grid_probe_counts(plan, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    rows = _level_rows(plan, "neutral", 17)
    for n, begin in ((700, 0), (4097, 12_345)):
        plain = E.probe_grid(_params(plan), SEED, STREAM, begin, n, MONTHS, rows).cpu().numpy()
        counts, years, launches = _probe(plan, "neutral", MONTHS, rows, n, begin)
        assert launches == 2 and np.array_equal(counts, plain)
        assert np.all(years[:, :, :, 1:] == 0) and np.all(years[:, :, 0, N.MCR_RULE_ALIVE] <= n)
        assert np.any((plain[:, :, 0] > 0) & (plain[:, :, 0] < n))


# ---- 3. against the CPU oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,wm", [("realized", 120), ("annual", 7), ("streams", 0)])
def test_a_cell_per_plan_equals_the_cpu_model(plan, wm, monkeypatch):
    """The cell at the plan's calibrated (month, level) under the symmetric rule over paths [0, 192): its success count and year
    counts are what the CPU model gives, path by path from the unmodified oracle.  A path with a year the model cannot decide
    (`verify`) would be dropped from both sides; at most 2 may be."""
    monkeypatch.delenv(KNOB, raising=False)
    n, rname = 192, "symmetric"
    rule = M.RULES[rname]
    level = M.LEVELS[plan, wm][rname]
    cfg = dict(M.plan_config(plan, REPO, wm))
    p = params_from_config(Config(**dict(cfg, monthly_expenses=level)))
    rows, flags, dropped = [], [], []
    for i in range(n):
        row, run = M.model(p, wm, rule, SEED, STREAM, i)
        outcome = {"success": run["success"][0], "years_to_ruin": run["years_to_ruin"][0], "final_balance": run["final_balance"][0]}
        if M.verify(p, wm, rule, SEED, STREAM, i, row, outcome):
            dropped.append(i)
        rows.append(row)
        flags.append(bool(run["success"][0]))
    assert len(dropped) <= 2, dropped
    months = [wm + 12, wm]                      # the cell is the second row; the grid's block is the plan's own
    base = params_from_config(Config(**cfg))
    levels = [[level], [level]]
    counts, years = E.probe_rule_grid(base, SEED, STREAM, 0, n, months, levels, SpendingRule(*rule))
    assert _launches() == 1
    counts, years = counts.cpu().numpy(), years.cpu().numpy()
    for i in dropped:                           # an undecidable path leaves both sides: the engine's own row of it
        one = E.run_rule_host(p, SEED, STREAM, i, 1, wm, SpendingRule(*rule))
        counts[1, 0] -= one["counters"].astype(np.int64)
        years[1, 0] -= one["year_counts"].astype(np.int64)
    keep = [i for i in range(n) if i not in dropped]
    want_years = M.year_counts_of(np.array([rows[i] for i in keep]).T, rule)
    assert counts[1, 0].tolist() == [sum(flags[i] for i in keep), len(keep)]
    assert np.array_equal(years[1, 0], want_years)
    assert want_years[:, N.MCR_RULE_CUT].sum() > 0 and want_years[:, N.MCR_RULE_FLOOR].sum() > 0 and want_years[:, N.MCR_RULE_RAISED].sum() > 0


# ---- 4. the fallback routes -------------------------------------------------------------------------------------------------------
def test_one_distinct_month_takes_the_rule_probe_per_row(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    plan, rname, n = "streams", "symmetric", 700
    for months in ([7], [7, 7, 7]):
        rows = _level_rows(plan, rname, 4, months)
        want_counts, want_years = _want(plan, rname, months, rows, n, 0)
        counts, years, launches = _probe(plan, rname, months, rows, n, 0)
        assert launches == 0 and np.array_equal(counts, want_counts) and np.array_equal(years, want_years)
    assert want_years[:, :, :, N.MCR_RULE_CUT].sum() > 0


def test_more_distinct_months_than_a_sweep_snapshots_take_the_rule_probe_per_row(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    plan, rname, n = "realized", "cut_only", 700
    months = list(range(0, 33))
    assert len(months) == 32 + 1                       # MCR_MAX_PROBE_CANDIDATES distinct months is what one sweep snapshots
    cal = _calibrated(plan, 0, rname)
    rows = [[cal, round(cal * (0.8 + 0.01 * c), 2)] for c in range(len(months))]
    want_counts, want_years = _want(plan, rname, months, rows, n, 0)
    counts, years, launches = _probe(plan, rname, months, rows, n, 0)
    assert launches == 0 and np.array_equal(counts, want_counts) and np.array_equal(years, want_years)
    # one month fewer: the shared route, the same integers
    counts, years, launches = _probe(plan, rname, months[:32], rows[:32], n, 0)
    assert launches == 1 and np.array_equal(counts, want_counts[:32]) and np.array_equal(years, want_years[:32])


def test_what_the_rule_launch_refuses_is_refused_by_its_words():
    import ctypes as C

    import torch

    many = dict(M.plan_config("realized", REPO))
    many["other_income_streams"] = [{"name": f"s{k}", "monthly_amount_today": 100.0 + k, "start_at_age": 50.0 + k, "duration_years": None,
                                     "inflation_indexed": True, "tax_rate": 0.1} for k in range(17)]
    p17 = params_from_config(Config(**many))
    assert p17.n_streams == 17
    rule = SpendingRule(*M.RULES["symmetric"])
    with pytest.raises(RuntimeError, match="code -4"):
        E.run_rule(p17, SEED, STREAM, 0, 700, 7, rule)
    single = N.last_error()
    assert "17 income streams" in single
    counts = torch.full((2, 2, 2), -7, dtype=torch.int64, device="cuda:0")
    years = torch.full((2, 2, RY, 4), -7, dtype=torch.int64, device="cuda:0")
    rng, rec = N.philox_rng(SEED), rule.record()
    marr, larr = (C.c_int32 * 2)(7, 120), (C.c_double * 4)(1000.0, 2000.0, 1000.0, 2000.0)
    rc = N.load_library().mcr_probe_rule_grid_rng(C.byref(p17), C.byref(rng), STREAM, 0, 700, marr, 2, larr, 2, C.byref(rec),
                                                  counts.data_ptr(), years.data_ptr(), 0, None)
    torch.cuda.synchronize()
    assert rc == N.MCR_ERR_UNSUPPORTED and N.last_error() == single and _launches() == 0
    assert bool((counts == -7).all()) and bool((years == -7).all())


def test_minimum_wave_knob_takes_the_rule_probe_per_row():
    """The knob is read per call; set high in a child process, the same grid takes the per-row route and counts the same."""
    plan, rname, n = "annual", "symmetric", 700
    rows = _level_rows(plan, rname, 4)
    want_counts, want_years = _want(plan, rname, MONTHS, rows, n, 0)
    code = ("import json, sys\n"
            "sys.path.insert(0, 'tests')\n"
            "import spending_rule_model as M\n"
            "from monte_carlo_retirement_amd import Config, params_from_config, _native as N, engine as E\n"
            "from monte_carlo_retirement_amd.spending_rules import SpendingRule\n"
            f"p = params_from_config(Config(**M.plan_config({plan!r}, '.')))\n"
            f"c, y = E.probe_rule_grid(p, M.SEED, M.STREAM, 0, {n}, {MONTHS!r}, {rows!r}, SpendingRule(*M.RULES[{rname!r}]))\n"
            "print(json.dumps([c.cpu().tolist(), y.cpu().tolist(), int(N.load_library().mcr_probe_rule_grid_last_fanout_launches())]))\n")
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], cwd=REPO, capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, **{KNOB: NEVER}))
    assert r.returncode == 0, r.stderr[-3000:]
    counts, years, launches = json.loads(r.stdout.strip().splitlines()[-1])
    assert launches == 0 and np.array_equal(np.array(counts), want_counts) and np.array_equal(np.array(years), want_years)


# ---- 5. the Python layer ----------------------------------------------------------------------------------------------------------
def _simulator(plan="realized", **over):
    return RetirementMonteCarloSimulator(Config(**dict(_plan_dict(plan), **over)), main_seed_override=SEED)


def test_grid_with_rule_rows_are_the_one_month_calls(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    sim = _simulator()
    rule = SpendingRule(*M.RULES["symmetric"])
    months = [120, 0, 7]
    levels = [M.LEVELS["realized", 7]["symmetric"], M.LEVELS["realized", 120]["symmetric"], 0.0]
    grid = sim.success_probability_grid_with_rule(months, rule, levels, 700)
    assert _launches() == 1 and grid.shape == (3, 3)
    for c, wm in enumerate(months):
        assert grid[c].tolist() == sim.success_probability_with_rule(wm, rule, levels, 700).tolist()
    assert len(set(grid.ravel().tolist())) >= 4 and np.all(grid[:, 2] == 100.0)
    one = sim.success_probability_grid_with_rule(months, rule, None, 700)
    assert one.shape == (3, 1)
    assert one[:, 0].tolist() == [sim.success_probability_with_rule(wm, rule, None, 700) for wm in months]


def _search_config():
    """A plan whose month search brackets, bisects and verifies within a few probes of 3 000 paths."""
    return dict(M.plan_config("realized", REPO), monthly_expenses=3500.0, num_simulations_search=3000, target_probability=85.0,
                starting_working_months_search=0)


def test_month_search_under_a_rule(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    rule = SpendingRule(*M.RULES["symmetric"])
    cfg = _search_config()
    sim = RetirementMonteCarloSimulator(Config(**cfg), main_seed_override=SEED)
    events = []
    months, prob, curve = sim.find_minimum_working_months_with_rule(rule, verbose=False, progress_callback=events.append)
    assert months > 0 and prob >= 85.0 and len(curve) >= 5
    for entry in curve:             # every entry is the one-month method on the search stream, rounded as the curve rounds
        assert entry["probability"] == round(sim.success_probability_with_rule(entry["working_months"], rule, None, 3000), 2), entry
    # the neutral rule: exactly the fixed-spending search
    e0, e1 = [], []
    fixed = RetirementMonteCarloSimulator(Config(**cfg), main_seed_override=SEED).find_minimum_working_months(verbose=False, progress_callback=e0.append)
    neutral = RetirementMonteCarloSimulator(Config(**cfg), main_seed_override=SEED).find_minimum_working_months_with_rule(
        SpendingRule.neutral(), verbose=False, progress_callback=e1.append)
    assert neutral == fixed and e0 == e1


def test_frontier_under_a_rule_is_the_single_month_searches(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    rule = SpendingRule(*M.RULES["symmetric"])
    cfg = dict(M.plan_config("realized", REPO), num_simulations_search=2000, target_probability=85.0)
    months = [0, 120]
    both = RetirementMonteCarloSimulator(Config(**cfg), main_seed_override=SEED).find_maximum_initial_expenses_by_months(months, rule, verbose=False)
    for wm, got in zip(months, both):
        one = RetirementMonteCarloSimulator(Config(**cfg), main_seed_override=SEED).find_maximum_initial_expenses(wm, rule, verbose=False)
        assert tuple(got) == tuple(one), wm
    assert 0.0 < both[0][0] < both[1][0]


# ---- 6. two ranks -----------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_hold_the_single_process_matrix(tmp_path):
    from rule_grid_dist_worker import MONTHS as D_MONTHS, N_PATHS as N_DIST, make_simulator, matrices

    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   OMP_NUM_THREADS="1")
        env.pop(KNOB, None)
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                       os.path.join(REPO, "tests", "rule_grid_dist_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        stdout, _ = p.communicate(timeout=600)
        assert p.returncode == 0, stdout.decode()[-3000:]
    res = [json.load(open(f"{out}.{r}")) for r in range(2)]
    want = matrices(make_simulator())
    assert want["by_path_range"] == want["by_candidate"] and len({x for row in want["by_path_range"] for x in row}) >= 4
    for r in res:
        assert r["matrices"] == want
    # sharded by path range, both ranks probe every row on their half; split by candidate, each rank takes every other row
    assert sorted((r["by_path_range"][0], r["by_path_range"][1]) for r in res) == [(0, 602), (602, 601)]
    assert all(r["by_path_range"][2] == D_MONTHS for r in res)
    assert sorted(tuple(r["by_candidate"][2]) for r in res) == sorted([tuple(D_MONTHS[0::2]), tuple(D_MONTHS[1::2])])
    assert all(r["by_candidate"][:2] == [0, N_DIST] for r in res)


# ---- the command line -------------------------------------------------------------------------------------------------------------
RULE_TEXT = "1.2,0.8,0.1,0.1,0.5,1.5"


def _cli(*flags):
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--seed", "7", "--search-paths", "3000", "--spending-rule", RULE_TEXT, *flags]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300, env={k: v for k, v in os.environ.items() if k != KNOB})
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _cli_simulator():
    from monte_carlo_retirement_amd import load_config_from_json

    raw = load_config_from_json(os.path.join(REPO, "scenarios", "config.json"))
    return RetirementMonteCarloSimulator(Config(**dict(raw, num_simulations_search=3000)), main_seed_override=7)


def test_cli_earliest_retirement_prints_both_month_searches():
    out = _cli("--earliest-retirement")
    rule = SpendingRule.parse(RULE_TEXT)
    fixed = _cli_simulator().find_minimum_working_months(verbose=False)
    ruled = _cli_simulator().find_minimum_working_months_with_rule(rule, verbose=False)
    assert out["rule"] == rule.as_dict()
    assert out["fixed_spending"] == {"working_months": fixed[0], "probability": fixed[1], "months_evaluated": len(fixed[2])}
    assert out["with_spending_rule"] == {"working_months": ruled[0], "probability": ruled[1], "months_evaluated": len(ruled[2])}
    assert out["months_sooner"] == fixed[0] - ruled[0] and ruled[0] != fixed[0]      # (the rule reached the search)


def test_cli_frontier_adds_the_rules_frontier_beside_the_fixed_one():
    out = _cli("--frontier", "180,240")
    rule = SpendingRule.parse(RULE_TEXT)
    fixed = _cli_simulator().find_maximum_monthly_expenses_by_months([180, 240], verbose=False)
    ruled = _cli_simulator().find_maximum_initial_expenses_by_months([180, 240], rule, verbose=False)
    assert [row["working_months"] for row in out] == [180, 240]
    for row, f, r in zip(out, fixed, ruled):
        assert (row["max_monthly_expenses"], row["probability"], row["levels_evaluated"]) == (f[0], f[1], len(f[2]))
        assert row["with_spending_rule"] == {"max_initial_monthly_expenses": r[0], "probability": r[1], "levels_evaluated": len(r[2])}
        assert r[0] != f[0] and f[0] > 0.0                                           # (the rule reached the search)
