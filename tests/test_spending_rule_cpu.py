"""Spending rules without a GPU: the ABI's two new structs as a C compiler lays them out, the host-side validation, the entry
point's loud failure without a device, the oracle-only model of the rule and its verifier (tests/spending_rule_model.py), the
search plumbing of `find_maximum_initial_expenses` and the arithmetic of `SpendingRuleOutcomes`."""

from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.spending_rules import SpendingRule, SpendingRuleOutcomes

import spending_rule_model as M

SEED, STREAM = 20260, 1


@pytest.fixture(scope="module")
def lib():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    return N.load_library()


def test_struct_layout_matches_what_a_c_compiler_sees(tmp_path):
    """sizeof / offsetof of both new ABI structs as gcc lays them out from include/mcr.h (C99) vs the ctypes mirrors."""
    structs = {"mcr_spending_rule": N.McrSpendingRule, "mcr_rule_outputs": N.McrRuleOutputs}
    lines = []
    for cname, T in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in T._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("columns %d %d %d %d %d\\n", MCR_RULE_ALIVE, MCR_RULE_CUT, MCR_RULE_FLOOR, MCR_RULE_RAISED, MCR_RULE_N_COUNTS);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    seen = dict(line.split() for line in out[:-1])
    for cname, T in structs.items():
        assert int(seen[cname]) == C.sizeof(T), cname
        for fname, _ in T._fields_:
            assert int(seen[f"{cname}.{fname}"]) == getattr(T, fname).offset, f"{cname}.{fname}"
    assert out[-1].split()[1:] == [str(v) for v in (N.MCR_RULE_ALIVE, N.MCR_RULE_CUT, N.MCR_RULE_FLOOR, N.MCR_RULE_RAISED, N.MCR_RULE_N_COUNTS)]
    assert C.sizeof(N.McrSpendingRule) == 48 and C.sizeof(N.McrRuleOutputs) == 24


GOOD = dict(upper=1.2, lower=0.8, cut=0.10, raise_=0.10, floor=0.5, ceiling=1.5)
BAD = [("upper", 0.999), ("upper", float("nan")), ("upper", float("inf")), ("lower", -0.01), ("lower", 1.01), ("lower", float("nan")),
       ("cut", -0.1), ("cut", 1.0), ("cut", float("nan")), ("raise_", -0.01), ("raise_", float("inf")), ("raise_", float("nan")),
       ("floor", -0.1), ("floor", 1.1), ("floor", float("nan")), ("ceiling", 0.9), ("ceiling", float("inf")), ("ceiling", float("nan"))]


def test_validation_names_the_field(lib):
    """Every range of include/mcr.h is enforced on the host (no device), with the field named in the error."""
    assert SpendingRule(**GOOD).as_dict()["raise"] == 0.10
    assert SpendingRule.neutral().is_neutral and not SpendingRule(**GOOD).is_neutral
    assert SpendingRule.parse("1.0, 0, 0.10, 0, 0.6, 1") == SpendingRule(1.0, 0.0, 0.10, 0.0, 0.6, 1.0)
    for values in M.RULES.values():
        rec = SpendingRule(*values).record()
        assert lib.mcr_validate_spending_rule(C.byref(rec)) == 0
    for field, value in BAD:
        cname = field.rstrip("_")
        rec = N.McrSpendingRule()
        for k, v in GOOD.items():
            setattr(rec, k.rstrip("_"), v)
        setattr(rec, cname, value)
        assert lib.mcr_validate_spending_rule(C.byref(rec)) == N.MCR_ERR_INVALID_ARG, (field, value)
        assert cname in N.last_error(), (field, value, N.last_error())
        with pytest.raises(ValueError, match=cname):
            SpendingRule(**dict(GOOD, **{field: value}))
    assert lib.mcr_validate_spending_rule(None) == N.MCR_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        SpendingRule.parse("1,2,3")
    with pytest.raises(Exception):
        SpendingRule.neutral().upper = 2.0      # frozen


def _child(code: str) -> str:
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_rule_launch_without_a_device_fails_loudly(lib):
    """There is no CPU fallback: without a HIP device mcr_run_rule_rng returns MCR_ERR_NO_DEVICE.  (In a child process: a call
    that initialises the HIP runtime would hold the GPU open for the rest of the session.)  With a device, the same call with
    no outputs requested and no paths succeeds."""
    out = _child("import ctypes as C, json\n"
                 "from monte_carlo_retirement_amd import Config, params_from_config\n"
                 "from monte_carlo_retirement_amd import _native as N\n"
                 "lib = N.load_library()\n"
                 "p = params_from_config(Config(**json.load(open('tests/golden/paths_injected.json'))[0]['cfg']))\n"
                 "rule, rng, o, ro = N.McrSpendingRule(1.2, 0.8, 0.1, 0.1, 0.5, 1.5), N.philox_rng(1), N.McrOutputs(), N.McrRuleOutputs()\n"
                 "rc = lib.mcr_run_rule_rng(C.byref(p), C.byref(rng), 1, 0, 0, 12, C.byref(rule), C.byref(o), C.byref(ro), 0, None)\n"
                 "print(lib.mcr_device_count(), rc, N.last_error().replace(' ', '_') or '-')")
    devices, rc, msg = out.split()[-3:]
    if int(devices) > 0:
        assert int(rc) == 0, msg
    else:
        assert int(rc) == N.MCR_ERR_NO_DEVICE and "no_usable_HIP_device" in msg, (rc, msg)


# ---- the model and its verifier, on the oracle alone ----------------------------------------------------------------------
N_MODEL = 32


@pytest.fixture(scope="module")
def plan(oracle):
    cfg = dict(M.plan_config("realized", REPO, 7), monthly_expenses=M.LEVELS["realized", 7]["symmetric"])
    return params_from_config(Config(**cfg)), 7


@pytest.fixture(scope="module")
def modelled(plan):
    """`model` of 32 paths under the symmetric rule: (row, run) per path, computed once."""
    p, wm = plan
    return [M.model(p, wm, M.RULES["symmetric"], SEED, STREAM, i) for i in range(N_MODEL)]


def _outcome(run):
    return {"success": run["success"][0], "years_to_ruin": run["years_to_ruin"][0], "final_balance": run["final_balance"][0]}


def test_model_under_the_neutral_rule_is_the_plain_oracle_run(oracle, plan):
    p, wm = plan
    plain = oracle.run_batch(p, SEED, STREAM, 0, N_MODEL, wm)
    for i in range(N_MODEL):
        row, run = M.model(p, wm, M.RULES["neutral"], SEED, STREAM, i)
        for k, v in run.items():
            if k in ("counters", "wr_obs_counts", "ruin_year_bins"):
                continue
            assert np.array_equal(v[..., 0], plain[k][..., i], equal_nan=True), (i, k)
        ytr = plain["years_to_ruin"][i]
        assert all((np.isnan(row[y]) and not M.begins_year(ytr, y)) or row[y] == 1.0 for y in range(p.retirement_years)), (i, row)
    assert int(plain["counters"][0]) < N_MODEL          # some of these paths fail: their rows end in NaN


def test_verify_accepts_the_models_rows(plan, modelled):
    p, wm = plan
    rule = M.RULES["symmetric"]
    rows = np.stack([row for row, _ in modelled], axis=1)
    undecidable = [M.verify(p, wm, rule, SEED, STREAM, i, row, _outcome(run)) for i, (row, run) in enumerate(modelled)]
    assert not any(undecidable)
    counts = M.year_counts_of(rows, rule)
    # the rule fires in both directions on these paths, and paths both fail and survive
    assert counts[:, N.MCR_RULE_CUT].sum() > 0 and counts[:, N.MCR_RULE_RAISED].sum() > 0
    assert 0 < counts[-1, N.MCR_RULE_ALIVE] < N_MODEL
    assert np.all(rows[0] == 1.0)


def _first_decision(row, kinds):
    """The first year y >= 1 whose multiplier differs from the year before (a decision that moved it) / equals it."""
    for y in range(1, len(row)):
        if np.isnan(row[y]):
            break
        if (row[y] != row[y - 1]) in kinds:
            return y
    return None


def test_verify_rejects_a_flipped_decision(plan, modelled):
    """One decision flipped (a cut not taken, or a cut taken where the rule keeps): the row no longer follows the rule."""
    p, wm = plan
    rule = M.RULES["symmetric"]
    rejected = 0
    for i, (row, run) in enumerate(modelled):
        for kinds in ((True,), (False,)):
            y = _first_decision(row, kinds)
            if y is None:
                continue
            bad = row.copy()
            bad[y] = row[y - 1] if row[y] != row[y - 1] else M.apply(rule, row[y - 1], M.CUT)
            with pytest.raises(AssertionError):
                M.verify(p, wm, rule, SEED, STREAM, i, bad, _outcome(run))
            rejected += 1
    assert rejected >= N_MODEL


def test_verify_rejects_a_multiplier_off_by_one_step(plan, modelled):
    """The decision's direction is right but the multiplier is one step further than the rule's arithmetic gives."""
    p, wm = plan
    rule = M.RULES["symmetric"]
    rejected = 0
    for i, (row, run) in enumerate(modelled):
        y = _first_decision(row, (True,))
        if y is None:
            continue
        bad = row.copy()
        step = M.CUT if row[y] < row[y - 1] else M.RAISE
        bad[y] = M.apply(rule, row[y], step)
        assert bad[y] != row[y]
        with pytest.raises(AssertionError):
            M.verify(p, wm, rule, SEED, STREAM, i, bad, _outcome(run))
        rejected += 1
    assert rejected >= N_MODEL // 2


def test_verify_rejects_a_wrong_outcome(plan, modelled):
    p, wm = plan
    row, run = modelled[0]
    out = _outcome(run)
    with pytest.raises(AssertionError):
        M.verify(p, wm, M.RULES["symmetric"], SEED, STREAM, 0, row, dict(out, success=not out["success"]))
    with pytest.raises(AssertionError):
        M.verify(p, wm, M.RULES["symmetric"], SEED, STREAM, 0, row, dict(out, final_balance=out["final_balance"] * (1 + 1e-6) + 1.0))


# ---- search plumbing --------------------------------------------------------------------------------------------------------
def test_find_maximum_initial_expenses_search_plumbing():
    """`find_maximum_initial_expenses` runs `spending.search_maximum_expenses` on `success_probability_with_rule`: a synthetic
    monotone probe in its place is searched to the resolution, on the search stream, with the rule and path count passed on."""
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = Config(**dict(M.plan_config("realized", REPO), num_simulations_search=2000, target_probability=85.0))
    sim = RetirementMonteCarloSimulator(cfg, main_seed_override=5)
    rule = SpendingRule(*M.RULES["cut_only"])
    calls = []

    def fake(working_months, rule_, monthly_expenses=None, num_simulations=None):
        calls.append((working_months, rule_, list(monthly_expenses), num_simulations, sim._stream_name))
        return np.array([90.0 if x <= 3456.78 else 10.0 for x in monthly_expenses])

    sim.success_probability_with_rule = fake
    events = []
    x, prob, curve = sim.find_maximum_initial_expenses(120, rule, resolution=1.0, verbose=False, progress_callback=events.append)
    assert x <= 3456.78 < x + 1.0 + 1e-9 and prob == 90.0
    assert all(c[0] == 120 and c[1] is rule and c[3] == 2000 and c[4] == "search" and 1 <= len(c[2]) <= N.MCR_MAX_EXPENSE_FANOUT for c in calls)
    assert calls[0][2][0] == 0.0 and len(curve) == sum(len(c[2]) for c in calls) == len(events)
    sim.success_probability_with_rule = lambda *a, **k: np.array([40.0 for _ in a[2]])
    assert sim.find_maximum_initial_expenses(120, rule, verbose=False)[:2] == (-1.0, 40.0)


# ---- outcomes arithmetic ----------------------------------------------------------------------------------------------------
def test_spending_rule_outcomes_arithmetic():
    counts = [[8, 0, 0, 0], [8, 4, 0, 1], [6, 3, 2, 0], [4, 4, 4, 0]]
    o = SpendingRuleOutcomes(3, 8, counts, 60.5, ever_cut=5)
    assert o.retirement_years == 4 and o.probability == 37.5
    assert o.alive_share.tolist() == [1.0, 1.0, 0.75, 0.5]
    assert o.cut_share.tolist() == [0.0, 0.5, 0.375, 0.5]
    assert o.floor_share.tolist() == [0.0, 0.0, 0.25, 0.5]
    assert o.raised_share.tolist() == [0.0, 0.125, 0.0, 0.0]
    assert o.ages.tolist() == [60.5, 61.5, 62.5, 63.5]
    assert o.ever_cut_share == 0.625
    doc = o.row()
    assert doc["probability"] == 37.5 and doc["ever_cut_share"] == 0.625 and len(doc["years"]) == 4
    assert doc["years"][2] == {"year": 2, "age": 62.5, "alive": 0.75, "cut": 0.375, "at_floor": 0.25, "raised": 0.0}
    plain = SpendingRuleOutcomes(3, 8, counts, 60.5)
    assert "ever_cut_share" not in plain.row() and plain != o and plain == SpendingRuleOutcomes(3, 8, np.array(counts), 60.5)
    with pytest.raises(ValueError, match="multiplier rows"):
        plain.ever_cut_share
    for bad in ([[9, 0, 0, 0]], [[4, 5, 0, 0]], [[4, 1, 2, 0]], [[4, -1, 0, 0]], [4, 0, 0, 0]):
        with pytest.raises(ValueError):
            SpendingRuleOutcomes(1, 8, bad, 60.0)
    with pytest.raises(ValueError):
        SpendingRuleOutcomes(9, 8, counts, 60.0)
