"""The rule probes (`mcr_probe_rules_rng`, `..._joint_rng`, `..._outcomes_rng`; path_kernel's PHASE 11) on the GPU, held to
`mcr_run_rule_rng`: one plain rule launch per option with the option's three amounts and its rule.  The existing tests hold that
launch to the unmodified CPU oracle on these plans, levels and seed (tests/test_gpu_spending_rule.py).

600 paths (ten 64-path fan-out workgroups, the last with 24 live lanes), 30 retirement years, working_months in {0, 7, 120}, the
plans `realized`, `annual`, `streams` of `spending_rule_model.plan_config`.  17 options per case, i.e. two fan-out launches of
unequal groups (9 + 8): each of the three rules of `spending_rule_model.RULES` at its calibrated level and at 0.7 x and 1.15 x
of it (9), each rule once more with a larger initial balance and once with half the contribution (6: the probe replaces all
three amounts, and the levels alone would never show it), an exact duplicate of option 4, and one neutral option (rule None).
Every comparison is of integers or of bit patterns: equality, no tolerance.
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
N_PATHS, RY, N_OPTIONS = 600, 30, 17
PLANS = ("realized", "annual", "streams")
MONTHS = (0, 7, 120)
CASES = [(plan, wm) for plan in PLANS for wm in MONTHS]
SEED, STREAM = M.SEED, M.STREAM
NEVER = str(1 << 40)          # MCR_RULE_FANOUT_MIN_WAVES: no batch has this many path-wavefronts
SENTINEL = -7
_cache = {}


def _config(plan, wm, **amounts):
    return Config(**dict(M.plan_config(plan, REPO, wm), **amounts))


def _base(plan, wm):
    """The parameter block every probe of a case is called with (the options replace its three amounts)."""
    return params_from_config(_config(plan, wm))


def _options(plan, wm):
    """The case's 17 options as ``(initial_balance, monthly_contribution, monthly_expenses, rule name or None)``."""
    cfg = _config(plan, wm)
    b0, c0 = float(cfg.initial_balance), float(cfg.monthly_contribution)
    options = []
    for rname in ("neutral", "cut_only", "symmetric"):
        level = M.LEVELS[plan, wm][rname]
        options += [(b0, c0, level * f, rname) for f in (1.0, 0.7, 1.15)]
        options += [(b0 * 1.25, c0, level, rname), (b0, c0 * 0.5, level, rname)]
    options.append(options[4])
    options.append((b0, c0, M.LEVELS[plan, wm]["cut_only"], None))
    assert len(options) == N_OPTIONS
    return options


def _records(options):
    return [(b, c, e, None if r is None else SpendingRule(*M.RULES[r])) for b, c, e, r in options]


def _reference(plan, wm):
    """Per option of the case: the count-only and the summary `mcr_run_rule_rng` launch, run once and shared (read only)."""
    if (plan, wm) not in _cache:
        count, summary = [], []
        for b, c, e, r in _options(plan, wm):
            p = params_from_config(_config(plan, wm, initial_balance=b, monthly_contribution=c, monthly_expenses=e))
            rule = SpendingRule(*M.RULES[r or "neutral"])
            count.append(E.run_rule_host(p, SEED, STREAM, 0, N_PATHS, wm, rule))
            summary.append(E.run_rule_host(p, SEED, STREAM, 0, N_PATHS, wm, rule, want="summary"))
        _cache[plan, wm] = (count, summary)
    return _cache[plan, wm]


def _launches():
    return int(N.load_library().mcr_probe_rules_last_fanout_launches())


def _bits(masks, n_paths):
    """int64 mask words [n, words] -> bool [n, n_paths]"""
    words = masks.cpu().numpy().view(np.uint64)
    bits = (words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(words.shape[0], -1).astype(bool)[:, :n_paths], bits.reshape(words.shape[0], -1).astype(bool)[:, n_paths:]


# ---- 1. counts and year counts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,wm", CASES)
def test_counts_and_year_counts_equal_the_rule_launches(plan, wm, monkeypatch):
    count, summary = _reference(plan, wm)
    want_counts = np.array([c["counters"] for c in count], dtype=np.int64)
    want_years = np.array([c["year_counts"] for c in count], dtype=np.int64)
    # the case is one where the options differ and the rules fire
    assert len({tuple(r) for r in want_counts.tolist()}) >= 5 and want_years[:, :, N.MCR_RULE_CUT].sum() > 0
    assert want_years[:, :, N.MCR_RULE_RAISED].sum() > 0 and want_years[:, :, N.MCR_RULE_FLOOR].sum() > 0
    assert all(s["counters"].tolist() == c["counters"].tolist() for s, c in zip(summary, count))
    p, records = _base(plan, wm), _records(_options(plan, wm))
    monkeypatch.delenv("MCR_RULE_FANOUT_MIN_WAVES", raising=False)
    counts, years = E.probe_rules(p, SEED, STREAM, 0, N_PATHS, wm, records)
    launches = _launches()
    assert counts.cpu().numpy().tolist() == want_counts.tolist()
    assert years.shape == (N_OPTIONS, RY, N.MCR_RULE_N_COUNTS) and np.array_equal(years.cpu().numpy(), want_years)
    # at most one frozen stream's lock column per wave: a launch's share is MCR_MAX_EXPENSE_FANOUT options
    assert launches >= 2 and launches == -(-N_OPTIONS // N.MCR_MAX_EXPENSE_FANOUT)
    # year counts not requested: the same counters
    counts_only, none = E.probe_rules(p, SEED, STREAM, 0, N_PATHS, wm, records, year_counts=False)
    assert none is None and counts_only.cpu().numpy().tolist() == want_counts.tolist()
    # the per-option route
    monkeypatch.setenv("MCR_RULE_FANOUT_MIN_WAVES", NEVER)
    counts, years = E.probe_rules(p, SEED, STREAM, 0, N_PATHS, wm, records)
    assert _launches() == 0
    assert counts.cpu().numpy().tolist() == want_counts.tolist() and np.array_equal(years.cpu().numpy(), want_years)
    # one option: the plain rule launch
    monkeypatch.delenv("MCR_RULE_FANOUT_MIN_WAVES")
    counts, years = E.probe_rules(p, SEED, STREAM, 0, N_PATHS, wm, records[5:6])
    assert _launches() == 0
    assert counts.cpu().numpy().tolist() == want_counts[5:6].tolist() and np.array_equal(years.cpu().numpy(), want_years[5:6])
    # no option: nothing
    counts, years = E.probe_rules(p, SEED, STREAM, 0, N_PATHS, wm, [])
    assert tuple(counts.shape) == (0, 2) and tuple(years.shape) == (0, RY, 4)


# ---- 2. neutral options -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,wm", CASES)
def test_neutral_options_count_what_the_scenario_probe_counts(plan, wm, monkeypatch):
    monkeypatch.delenv("MCR_RULE_FANOUT_MIN_WAVES", raising=False)
    options = _options(plan, wm)
    p = _base(plan, wm)
    scenarios = [o[:3] for o in options]
    plain = E.probe_scenarios(p, SEED, STREAM, 0, N_PATHS, wm, scenarios).cpu().numpy()
    for neutral in (None, SpendingRule.neutral()):
        counts, years = E.probe_rules(p, SEED, STREAM, 0, N_PATHS, wm, [s + (neutral,) for s in scenarios])
        assert _launches() == 2
        assert counts.cpu().numpy().tolist() == plain.tolist()
        years = years.cpu().numpy()
        assert np.all(years[:, :, 1:] == 0) and years[:, 0, N.MCR_RULE_ALIVE].max() <= N_PATHS
    assert plain[:, 0].min() < N_PATHS and len(set(plain[:, 0].tolist())) >= 5


# ---- 3. joint -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,wm", CASES)
def test_joint_masks_are_the_summary_launches_success_columns(plan, wm, monkeypatch):
    count, summary = _reference(plan, wm)
    success = np.array([s["success"] for s in summary]).astype(bool)             # [17, 600]
    want_joint = success.astype(np.int64) @ success.astype(np.int64).T
    want_extremes = [int(success.all(axis=0).sum()), int((~success).all(axis=0).sum())]
    p, records = _base(plan, wm), _records(_options(plan, wm))
    results = []
    for knob in (None, NEVER):
        if knob is None:
            monkeypatch.delenv("MCR_RULE_FANOUT_MIN_WAVES", raising=False)
        else:
            monkeypatch.setenv("MCR_RULE_FANOUT_MIN_WAVES", knob)
        counts, years, joint, extremes, masks = E.probe_rules_joint(p, SEED, STREAM, 0, N_PATHS, wm, records)
        assert _launches() == (2 if knob is None else 0)
        assert tuple(masks.shape) == (N_OPTIONS, 10)
        bits, tail = _bits(masks, N_PATHS)
        assert np.array_equal(bits, success) and not tail.any() and tail.shape[1] == 40
        assert np.array_equal(joint.cpu().numpy(), want_joint) and extremes.cpu().numpy().tolist() == want_extremes
        assert counts.cpu().numpy().tolist() == [c["counters"].tolist() for c in count]
        assert np.array_equal(years.cpu().numpy(), np.array([c["year_counts"] for c in count], dtype=np.int64))
        results.append((masks.cpu().numpy(), joint.cpu().numpy()))
        # masks kept by the library: the same matrix
        _, _, joint2, extremes2, none = E.probe_rules_joint(p, SEED, STREAM, 0, N_PATHS, wm, records, masks=None)
        assert none is None and np.array_equal(joint2.cpu().numpy(), want_joint) and extremes2.cpu().numpy().tolist() == want_extremes
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert 0 < want_extremes[0] + want_extremes[1] < N_PATHS


# ---- 4. outcomes ------------------------------------------------------------------------------------------------------------------
def _outcome_rows(p, wm, records, begin=0, n=N_PATHS, stride=640):
    import torch

    dev = torch.device("cuda", 0)
    fin = torch.full((len(records), stride), float(SENTINEL), dtype=torch.float64, device=dev)
    ruin = torch.full((len(records), stride), float(SENTINEL), dtype=torch.float64, device=dev)
    counts, years, fin2, ruin2 = E.probe_rules_outcomes(p, SEED, STREAM, begin, n, wm, records, final_balance=fin, years_to_ruin=ruin,
                                                        path_stride=stride)
    assert fin2 is fin and ruin2 is ruin
    return counts.cpu().numpy(), years.cpu().numpy(), fin.cpu().numpy(), ruin.cpu().numpy()


@pytest.mark.parametrize("plan,wm", CASES)
def test_outcome_rows_are_the_summary_launches_columns(plan, wm, monkeypatch):
    count, summary = _reference(plan, wm)
    want_final = np.array([np.where(s["success"].astype(bool), s["final_balance"], np.nan) for s in summary])
    want_ruin = np.array([s["years_to_ruin"] for s in summary])
    assert np.isnan(want_ruin).any() and (~np.isnan(want_ruin)).any()
    p, records = _base(plan, wm), _records(_options(plan, wm))
    results = []
    for knob in (None, NEVER):
        if knob is None:
            monkeypatch.delenv("MCR_RULE_FANOUT_MIN_WAVES", raising=False)
        else:
            monkeypatch.setenv("MCR_RULE_FANOUT_MIN_WAVES", knob)
        counts, years, fin, ruin = _outcome_rows(p, wm, records)
        assert _launches() == (2 if knob is None else 0)
        assert np.array_equal(fin[:, :N_PATHS].view(np.uint64), want_final.view(np.uint64))
        assert np.array_equal(ruin[:, :N_PATHS].view(np.uint64), want_ruin.view(np.uint64))
        assert np.all(fin[:, N_PATHS:] == SENTINEL) and np.all(ruin[:, N_PATHS:] == SENTINEL)
        assert counts.tolist() == [c["counters"].tolist() for c in count]
        assert np.array_equal(years, np.array([c["year_counts"] for c in count], dtype=np.int64))
        results.append((fin, ruin))
    assert np.array_equal(results[0][0].view(np.uint64), results[1][0].view(np.uint64))
    assert np.array_equal(results[0][1].view(np.uint64), results[1][1].view(np.uint64))


# ---- 5. partition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,wm", [("realized", 7), ("annual", 120), ("streams", 0)])
def test_partition_of_the_path_range(plan, wm, monkeypatch):
    """[0, 333) and [333, 600): counts and year counts sum to the whole range's, mask bits and outcome rows concatenate to it."""
    monkeypatch.delenv("MCR_RULE_FANOUT_MIN_WAVES", raising=False)
    p, records = _base(plan, wm), _records(_options(plan, wm))
    whole = E.probe_rules_joint(p, SEED, STREAM, 0, N_PATHS, wm, records)
    whole_rows = _outcome_rows(p, wm, records)
    parts, part_rows = [], []
    for begin, n in ((0, 333), (333, 267)):
        parts.append(E.probe_rules_joint(p, SEED, STREAM, begin, n, wm, records))
        assert _launches() == 2
        part_rows.append(_outcome_rows(p, wm, records, begin, n, stride=384))
    for k in (0, 1):     # counts, year counts
        assert np.array_equal(parts[0][k].cpu().numpy() + parts[1][k].cpu().numpy(), whole[k].cpu().numpy())
        assert np.array_equal(part_rows[0][k] + part_rows[1][k], whole_rows[k])
        assert np.array_equal(whole_rows[k], whole[k].cpu().numpy())
    bits = np.concatenate([_bits(parts[0][4], 333)[0], _bits(parts[1][4], 267)[0]], axis=1)
    assert np.array_equal(bits, _bits(whole[4], N_PATHS)[0])
    assert not _bits(parts[0][4], 333)[1].any() and not _bits(parts[1][4], 267)[1].any()
    for k in (2, 3):     # final_balance, years_to_ruin
        rows = np.concatenate([part_rows[0][k][:, :333], part_rows[1][k][:, :267]], axis=1)
        assert np.array_equal(rows.view(np.uint64), whole_rows[k][:, :N_PATHS].view(np.uint64))
        assert np.all(part_rows[0][k][:, 333:] == SENTINEL) and np.all(part_rows[1][k][:, 267:] == SENTINEL)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_bad_and_unsupported_requests_are_refused_by_name_and_compute_nothing():
    import torch

    plan, wm = "realized", 7
    p = _base(plan, wm)
    good = _records(_options(plan, wm))
    lib = N.load_library()
    dev = torch.device("cuda", 0)
    arr33, _ = E._rule_option_records([good[k % N_OPTIONS] for k in range(33)])

    def call(form, params, rng, options, n=None, null_joint=False):
        """One entry point with every output sentinel-filled: (rc, message, whether anything was written)."""
        arr, n_rec = options if isinstance(options, tuple) else E._rule_option_records(options)
        n_opt = n_rec if n is None else n
        words = int(E.joint_mask_words(N_PATHS))
        ints = {"counts": (n_opt, 2), "years": (n_opt, RY, 4), "masks": (n_opt, words), "joint": (n_opt, n_opt), "extremes": (2,)}
        ints = {k: torch.full(s, SENTINEL, dtype=torch.int64, device=dev) for k, s in ints.items()}
        rows = [torch.full((n_opt, 640), float(SENTINEL), dtype=torch.float64, device=dev) for _ in range(2)]
        rng = E._as_rng(rng, 0)
        head = (C.byref(params), C.byref(rng), STREAM, 0, N_PATHS, wm, arr, n_opt, ints["counts"].data_ptr(), ints["years"].data_ptr())
        if form == "plain":
            rc = lib.mcr_probe_rules_rng(*head, 0, None)
        elif form == "joint":
            rc = lib.mcr_probe_rules_joint_rng(*head, ints["masks"].data_ptr(), None if null_joint else ints["joint"].data_ptr(),
                                               ints["extremes"].data_ptr(), 0, None)
        else:
            out = N.McrOptionOutcomes(rows[0].data_ptr(), rows[1].data_ptr(), 640)
            rc = lib.mcr_probe_rules_outcomes_rng(*head, C.byref(out), 0, None)
        msg, launches = N.last_error(), _launches()
        torch.cuda.synchronize()
        touched = bool(any((t != SENTINEL).any() for t in ints.values()) or any((t != SENTINEL).any() for t in rows))
        return rc, msg, touched, launches

    for form in ("plain", "joint", "outcomes"):
        rc, msg, touched, launches = call(form, p, SEED, good)
        assert rc == 0 and touched and launches == 2, (form, rc, msg)            # the request itself is a valid one
    bad_rule = list(good)
    bad_rule[3] = good[3][:3] + (N.McrSpendingRule(1.2, 0.8, 1.0, 0.1, 0.5, 1.5),)           # cut = 1
    bad_floor = list(good)
    bad_floor[16] = good[16][:3] + (N.McrSpendingRule(1.2, 0.8, 0.1, 0.1, float("nan"), 1.5),)
    negative = list(good)
    negative[9] = (good[9][0], -1.0, good[9][2], good[9][3])
    infinite = list(good)
    infinite[0] = (good[0][0], good[0][1], float("inf"), good[0][3])
    history = N.history_rng(SEED, np.random.default_rng(1).standard_normal((240, 3)), 12)
    many = dict(M.plan_config(plan, REPO, wm))
    many["other_income_streams"] = [{"name": f"s{k}", "monthly_amount_today": 100.0 + k, "start_at_age": 50.0 + k, "duration_years": None,
                                     "inflation_indexed": True, "tax_rate": 0.1} for k in range(17)]
    p17 = params_from_config(Config(**many))
    assert p17.n_streams == 17
    INVALID, UNSUPPORTED = N.MCR_ERR_INVALID_ARG, N.MCR_ERR_UNSUPPORTED
    cases = [("a bad rule in options[3]", dict(params=p, rng=SEED, options=bad_rule), INVALID, "options[3].rule.cut"),
             ("a NaN floor in options[16]", dict(params=p, rng=SEED, options=bad_floor), INVALID, "options[16].rule.floor"),
             ("a negative amount", dict(params=p, rng=SEED, options=negative), INVALID, "options[9].monthly_contribution"),
             ("an infinite amount", dict(params=p, rng=SEED, options=infinite), INVALID, "options[0].monthly_expenses"),
             ("the NumPy stream", dict(params=p, rng=N.numpy_rng(12345), options=good), UNSUPPORTED, "NumPy stream"),
             ("the history stream", dict(params=p, rng=history, options=good), UNSUPPORTED, "history stream"),
             ("17 income streams", dict(params=p17, rng=SEED, options=good), UNSUPPORTED, "17 income streams")]
    for what, kw, code, word in cases:
        for form in ("plain", "joint", "outcomes"):
            rc, msg, touched, launches = call(form, **kw)
            assert rc == code and word in msg and not touched and launches == 0, (what, form, rc, msg, touched)
    # the joint call's own checks come first: the cap (before a bad option is looked at), a null joint
    rc, msg, touched, launches = call("joint", p, SEED, (arr33, 33))
    assert rc == INVALID and "MCR_MAX_JOINT_OPTIONS" in msg and not touched and launches == 0, (rc, msg)
    rc, msg, touched, launches = call("joint", p, SEED, good, null_joint=True)
    assert rc == INVALID and "joint" in msg and not touched and launches == 0, (rc, msg)
    with pytest.raises(RuntimeError, match="code -4"):
        E.probe_rules(p17, SEED, STREAM, 0, N_PATHS, wm, good)
    with pytest.raises(ValueError, match="MCR_MAX_JOINT_OPTIONS"):
        E.probe_rules_joint(p, SEED, STREAM, 0, N_PATHS, wm, [good[k % N_OPTIONS] for k in range(33)])


# ---- 7. the Python methods ------------------------------------------------------------------------------------------------------------
CLASS_PATHS, CLASS_WM = 3000, 233


def _class_simulator(**over):
    from rule_probe_dist_worker import make_simulator

    return make_simulator(**over)


def test_compare_spending_rules_is_the_per_option_methods():
    from rule_probe_dist_worker import OPTIONS

    sim = _class_simulator()
    doc = sim.compare_spending_rules(CLASS_WM, OPTIONS, CLASS_PATHS)
    assert [set(row) for row in doc["options"]] == [{"initial_balance", "monthly_contribution", "monthly_expenses", "rule", "probability",
                                                     "years"}] * len(OPTIONS)
    probs = sim.success_probability_by_rules(CLASS_WM, OPTIONS, CLASS_PATHS)
    assert probs.tolist() == [row["probability"] for row in doc["options"]]
    for option, row in zip(OPTIONS, doc["options"]):
        rule = SpendingRule.neutral() if option.get("rule") is None else SpendingRule(*option["rule"])
        one = _class_simulator(**{k: v for k, v in option.items() if k != "rule"})
        assert row["probability"] == one.success_probability_with_rule(CLASS_WM, rule, None, CLASS_PATHS)
        assert row["years"] == one.spending_rule_outcomes(CLASS_WM, rule, CLASS_PATHS).years()
        assert row["rule"] == (None if option.get("rule") is None else rule.as_dict())
        assert row["monthly_expenses"] == float(one.params_model.monthly_expenses)
        assert row["initial_balance"] == float(one.params_model.initial_balance)
    # options 0 and 1 are the same option and no other does as well: the first of equals
    assert doc["options"][0]["probability"] == doc["options"][1]["probability"] == max(probs) and doc["best"] == 0
    assert 0.0 < min(probs) < max(probs) and len(set(probs.tolist())) >= 4
    # --paired and --outcomes compose, on the same probabilities
    full = sim.compare_spending_rules(CLASS_WM, OPTIONS, CLASS_PATHS, paired=True, outcomes=True)
    paired = sim.compare_spending_rules(CLASS_WM, OPTIONS, CLASS_PATHS, paired=True)
    outcomes = sim.compare_spending_rules(CLASS_WM, OPTIONS, CLASS_PATHS, outcomes=True)
    joint = sim.joint_outcomes_by_rules(CLASS_WM, OPTIONS, CLASS_PATHS)
    per_option = sim.option_outcomes_by_rules(CLASS_WM, OPTIONS, CLASS_PATHS)
    assert joint.probabilities.tolist() == per_option.probabilities.tolist() == probs.tolist()
    for i, row in enumerate(full["options"]):
        assert {k: v for k, v in row.items() if k in doc["options"][i]} == doc["options"][i]
        assert row["vs_best"] == joint.difference(0, i) == paired["options"][i]["vs_best"]
        assert {k: row[k] for k in ("lasts_until_age", "median_ruin_age", "final_balance")} == per_option.row(i)
        assert outcomes["options"][i] == {k: v for k, v in row.items() if k != "vs_best"}
    assert full["best"] == 0 and 1 in full["tied_with_best"] and full["tied_with_best"] == joint.indistinguishable_from(0)
    assert (full["all_succeed"], full["none_succeed"]) == (joint.all_succeed, joint.none_succeed)
    assert "vs_best" not in outcomes["options"][0] and "final_balance" not in paired["options"][0]
    with pytest.raises(ValueError, match="unknown key"):
        sim.compare_spending_rules(CLASS_WM, [{"rule": None, "monthly_expense": 1.0}], CLASS_PATHS)
    assert sim.compare_spending_rules(CLASS_WM, [], CLASS_PATHS) == {"options": [], "best": None}


def test_levels_of_success_probability_with_rule_are_its_one_level_calls(monkeypatch):
    monkeypatch.delenv("MCR_RULE_FANOUT_MIN_WAVES", raising=False)
    sim = _class_simulator()
    rule = SpendingRule(*M.RULES["symmetric"])
    # 18 levels, two fan-out launches: no spending, and 13 000 .. 19 000, across which the CPU model of the symmetric rule goes from
    # every path succeeding to 2 % of them (tests/rule_probe_dist_worker.py)
    levels = [0.0] + [13000.0 + 375.0 * k for k in range(17)]
    many = sim.success_probability_with_rule(CLASS_WM, rule, levels, CLASS_PATHS)
    assert _launches() == 2
    ones = [sim.success_probability_with_rule(CLASS_WM, rule, x, CLASS_PATHS) for x in levels]
    assert isinstance(many, np.ndarray) and many.tolist() == ones
    assert many[0] == 100.0 and 0.0 < many[-1] < 100.0 and len(set(ones)) >= 6
    two = sim.success_probability_with_rule(CLASS_WM, rule, levels[5:7], CLASS_PATHS)
    assert two.tolist() == ones[5:7] and _launches() == 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_return_the_single_process_document(tmp_path):
    from rule_probe_dist_worker import N_PATHS as N_DIST, OPTIONS, WM, documents, make_simulator

    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   OMP_NUM_THREADS="1")
        env.pop("MCR_RULE_FANOUT_MIN_WAVES", None)
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                       os.path.join(REPO, "tests", "rule_probe_dist_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        stdout, _ = p.communicate(timeout=600)
        assert p.returncode == 0, stdout.decode()[-3000:]
    res = [json.load(open(f"{out}.{r}")) for r in range(2)]
    want = json.loads(json.dumps(documents(make_simulator(), OPTIONS, WM, N_DIST)))
    assert want["by_path_range"]["best"] == 0 and len(want["by_path_range"]["options"]) == len(OPTIONS)
    for r in res:
        assert r["documents"] == want
    # sharded by path range, both ranks probe every option on their half; split by option, each rank takes every other one
    assert sorted(tuple(r["by_path_range"]) for r in res) == [(0, 2502, len(OPTIONS)), (2502, 2501, len(OPTIONS))]
    assert sorted(tuple(r["by_option"]) for r in res) == [(0, N_DIST, 3), (0, N_DIST, 4)]


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_compare_rules_prints_the_methods_document():
    from monte_carlo_retirement_amd import load_config_from_json
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    text = "1.0,0,0.1,0,0.6,1; 1.2,0.8,0.1,0.1,0.5,1.5 ;none"
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--seed", "7", "--paths", "3000", "--working-months", str(CLASS_WM),
           "--compare-rules", text]
    env = {k: v for k, v in os.environ.items() if k != "MCR_RULE_FANOUT_MIN_WAVES"}
    r = subprocess.run(cmd + ["--paired", "--outcomes", "--full"], cwd=REPO, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    raw = load_config_from_json(os.path.join(REPO, "scenarios", "config.json"))
    sim = RetirementMonteCarloSimulator(Config(**dict(raw, num_simulations_main=3000)), main_seed_override=7)
    sim.use_final_seeds()
    rules = [M.RULES["cut_only"], M.RULES["symmetric"], None]
    want = json.loads(json.dumps(sim.compare_spending_rules(CLASS_WM, [{"rule": x} for x in rules], paired=True, outcomes=True)))
    assert {k: out[k] for k in want} == want and out["working_months"] == CLASS_WM and out["num_simulations"] == 3000
    assert [row["rule"] for row in out["options"]] == [SpendingRule(*M.RULES["cut_only"]).as_dict(), SpendingRule(*M.RULES["symmetric"]).as_dict(), None]
    # the table: a title, a header and one line per rule
    r = subprocess.run(cmd + ["--paired"], cwd=REPO, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()[-5:]
    assert f"best = #{want['best']}" in lines[0] and "vs best" in lines[1] and "fixed spending" in lines[4] and "1.2,0.8,0.1,0.1,0.5,1.5" in lines[3]
