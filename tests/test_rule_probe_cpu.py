"""The rule probes without a GPU: `mcr_rule_option` as a C compiler lays it out, the ABI version, the records `rule_options`
builds, the host-side validation of the entry points (it runs before the device is touched), their loud failure without a
device, and the document `compare_spending_rules` assembles from a faked probe."""

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
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.spending_rules import SpendingRule, SpendingRuleOutcomes, rule_options

import spending_rule_model as M

SYMMETRIC = (1.2, 0.8, 0.10, 0.10, 0.5, 1.5)


@pytest.fixture(scope="module")
def lib():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    return N.load_library()


def test_rule_option_layout_matches_what_a_c_compiler_sees(tmp_path):
    lines = ['printf("mcr_rule_option %zu\\n", sizeof(mcr_rule_option));']
    for fname, _ in N.McrRuleOption._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(mcr_rule_option, {fname}));')
    for fname, _ in N.McrSpendingRule._fields_:
        lines.append(f'printf("rule.{fname} %zu\\n", offsetof(mcr_rule_option, rule.{fname}));')
    lines.append('printf("abi %d\\n", MCR_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    seen = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(seen["mcr_rule_option"]) == C.sizeof(N.McrRuleOption) == 72
    for fname, _ in N.McrRuleOption._fields_:
        assert int(seen[fname]) == getattr(N.McrRuleOption, fname).offset, fname
    for fname, _ in N.McrSpendingRule._fields_:
        assert int(seen[f"rule.{fname}"]) == N.McrRuleOption.rule.offset + getattr(N.McrSpendingRule, fname).offset, fname
    assert N.McrRuleOption.rule.offset == 24
    assert int(seen["abi"]) == N.MCR_ABI_VERSION == 8


def test_abi_version_and_symbols(lib):
    assert lib.mcr_abi_version() == 8
    for sym in ("mcr_probe_rules_rng", "mcr_probe_rules_joint_rng", "mcr_probe_rules_outcomes_rng", "mcr_probe_rules_last_fanout_launches"):
        assert sym in N.ABI_SYMBOLS and hasattr(lib, sym)


def _config(**over):
    return Config(**dict(M.plan_config("realized", REPO), **over))


def test_rule_options_builds_the_records_and_rejects_unknown_keys():
    cfg = _config()
    b0, c0, e0 = float(cfg.initial_balance), float(cfg.monthly_contribution), float(cfg.monthly_expenses)
    rule = SpendingRule(*SYMMETRIC)
    records = rule_options(cfg, [{"rule": rule}, {"rule": SYMMETRIC, "monthly_expenses": 1234.5}, {"rule": None, "initial_balance": 1.0},
                                 {"monthly_contribution": 7}, {}])
    assert records == [(b0, c0, e0, rule), (b0, c0, 1234.5, rule), (1.0, c0, e0, None), (b0, 7.0, e0, None), (b0, c0, e0, None)]
    assert records[1][3] is not rule and all(isinstance(x, float) for r in records for x in r[:3])
    assert rule_options(cfg, []) == []
    with pytest.raises(ValueError, match=r"options\[1\]: unknown key\(s\) \['monthly_expense'\]"):
        rule_options(cfg, [{"rule": None}, {"rule": None, "monthly_expense": 1.0}])
    with pytest.raises(ValueError, match=r"options\[0\]\.rule.*upper"):
        rule_options(cfg, [{"rule": (0.9, 0.8, 0.1, 0.1, 0.5, 1.5)}])
    with pytest.raises(ValueError, match=r"options\[2\]\.rule"):
        rule_options(cfg, [{}, {}, {"rule": (1.2, 0.8, 0.1)}])
    # the engine's records: the three amounts and the rule's six values; None is the neutral rule
    arr, n = E._rule_option_records(records)
    assert n == 5 and C.sizeof(arr) == 5 * 72
    assert [getattr(arr[1].rule, k) for k in ("upper", "lower", "cut", "raise", "floor", "ceiling")] == list(SYMMETRIC)
    assert (arr[1].initial_balance, arr[1].monthly_contribution, arr[1].monthly_expenses) == (b0, c0, 1234.5)
    assert [getattr(arr[2].rule, k) for k in ("upper", "lower", "cut", "raise", "floor", "ceiling")] == [1.0, 1.0, 0.0, 0.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="every option is"):
        E._rule_option_records([(1.0, 2.0, 3.0)])


def _good(n=4):
    return [(240000.0, 5000.0, 1000.0 + k, SpendingRule(*SYMMETRIC)) for k in range(n)]


def _call(lib, form, params, rng, options, n=None, joint=1, stride=64, n_paths=64):
    """An entry point with addresses that are never followed: validation comes before the device and the outputs."""
    arr, n_rec = E._rule_option_records(options)
    head = (C.byref(params), C.byref(rng), 1, 0, n_paths, 12, arr, n_rec if n is None else n, 8, 8)
    if form == "plain":
        rc = lib.mcr_probe_rules_rng(*head, 0, None)
    elif form == "joint":
        rc = lib.mcr_probe_rules_joint_rng(*head, None, joint or None, None, 0, None)
    else:
        rows = N.McrOptionOutcomes(8, 8, stride)
        rc = lib.mcr_probe_rules_outcomes_rng(*head, C.byref(rows), 0, None)
    return rc, N.last_error()


def test_validation_names_the_field_on_the_host(lib):
    """Every check of the probes' arguments runs on the host, before the device is entered: each of these calls returns its
    code and names the field whether or not the box has a GPU, and follows none of the (bogus) output addresses."""
    p = params_from_config(_config())
    rng = N.philox_rng(1)
    rule = SpendingRule(*SYMMETRIC)

    def with_rule(k, **over):
        rec = rule.record()
        for f, v in over.items():
            setattr(rec, f, v)
        options = _good()
        options[k] = options[k][:3] + (rec,)
        return options

    def with_amount(k, i, v):
        options = _good()
        options[k] = tuple(v if j == i else x for j, x in enumerate(options[k]))
        return options

    bad = [(with_rule(3, upper=0.5), "options[3].rule.upper"), (with_rule(0, lower=1.5), "options[0].rule.lower"),
           (with_rule(1, cut=1.0), "options[1].rule.cut"), (with_rule(2, **{"raise": -0.1}), "options[2].rule.raise"),
           (with_rule(3, floor=float("nan")), "options[3].rule.floor"), (with_rule(3, ceiling=0.5), "options[3].rule.ceiling"),
           (with_amount(2, 0, -1.0), "options[2].initial_balance"), (with_amount(1, 1, float("nan")), "options[1].monthly_contribution"),
           (with_amount(3, 2, float("inf")), "options[3].monthly_expenses")]
    for form in ("plain", "joint", "outcomes"):
        for options, field in bad:
            rc, msg = _call(lib, form, p, rng, options)
            assert rc == N.MCR_ERR_INVALID_ARG and msg.startswith(field + " = "), (form, field, rc, msg)
        rc, msg = _call(lib, form, p, rng, _good(), n=-1)
        assert rc == N.MCR_ERR_INVALID_ARG and "n_options" in msg, (form, msg)
        rc, msg = _call(lib, form, p, N.numpy_rng(5), _good())
        assert rc == N.MCR_ERR_UNSUPPORTED and "NumPy stream" in msg, (form, msg)
        many = dict(M.plan_config("realized", REPO))
        many["other_income_streams"] = [{"name": f"s{k}", "monthly_amount_today": 100.0 + k, "start_at_age": 50.0 + k, "duration_years": None,
                                         "inflation_indexed": True, "tax_rate": 0.1} for k in range(17)]
        rc, msg = _call(lib, form, params_from_config(Config(**many)), rng, _good())
        assert rc == N.MCR_ERR_UNSUPPORTED and "17 income streams" in msg, (form, msg)
        assert lib.mcr_probe_rules_last_fanout_launches() == 0
    # the joint and the outcomes forms' own checks come first
    rc, msg = _call(lib, "joint", p, rng, with_rule(0, upper=0.5) * 9, n=33)
    assert rc == N.MCR_ERR_INVALID_ARG and "MCR_MAX_JOINT_OPTIONS" in msg, msg
    rc, msg = _call(lib, "joint", p, rng, _good(), joint=0)
    assert rc == N.MCR_ERR_INVALID_ARG and "null joint" in msg, msg
    rc, msg = _call(lib, "outcomes", p, rng, with_rule(0, upper=0.5), stride=63)
    assert rc == N.MCR_ERR_INVALID_ARG and "path_stride" in msg, msg


def _child(code: str) -> str:
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_rule_probe_without_a_device_fails_loudly(lib):
    """There is no CPU fallback: without a HIP device a valid call returns MCR_ERR_NO_DEVICE.  (In a child process: a call that
    initialises the HIP runtime would hold the GPU open for the rest of the session.)  With a device, the same call over no
    paths and with no year counts succeeds and zeroes its counters."""
    out = _child("import ctypes as C, json\n"
                 "from monte_carlo_retirement_amd import Config, params_from_config\n"
                 "from monte_carlo_retirement_amd import _native as N\n"
                 "from monte_carlo_retirement_amd import engine as E\n"
                 "lib = N.load_library()\n"
                 "p = params_from_config(Config(**json.load(open('tests/golden/paths_injected.json'))[0]['cfg']))\n"
                 "rule, rng = N.McrSpendingRule(1.2, 0.8, 0.1, 0.1, 0.5, 1.5), N.philox_rng(1)\n"
                 "arr, n = E._rule_option_records([(1e5, 100.0, 900.0, rule), (1e5, 100.0, 950.0, None)])\n"
                 "devices = lib.mcr_device_count()\n"
                 "if devices:\n"
                 "    import torch\n"
                 "    counts = torch.full((2, 2), -7, dtype=torch.int64, device='cuda:0')\n"
                 "    address = counts.data_ptr()\n"
                 "else:\n"
                 "    counts = (C.c_uint64 * 4)()\n"
                 "    address = C.addressof(counts)\n"
                 "rc = lib.mcr_probe_rules_rng(C.byref(p), C.byref(rng), 1, 0, 0, 12, arr, n, address, None, 0, None)\n"
                 "msg = N.last_error().replace(' ', '_') or '-'\n"
                 "zeroed = int(devices > 0 and bool((counts == 0).all().item()))\n"
                 "print(devices, rc, zeroed, msg)")
    devices, rc, zeroed, msg = out.split()[-4:]
    if int(devices) > 0:
        assert int(rc) == 0 and int(zeroed) == 1, (rc, msg)
    else:
        assert int(rc) == N.MCR_ERR_NO_DEVICE and "no_usable_HIP_device" in msg, (rc, msg)


def test_compare_spending_rules_assembles_the_document_from_the_probe():
    """`compare_spending_rules` on a faked probe: the rows, `best` as the first of equals, `paired` and `outcomes` composed from
    the joint and the per-option objects exactly as `compare_claiming_options` composes them."""
    from monte_carlo_retirement_amd.outcomes import OptionOutcomes
    from monte_carlo_retirement_amd.paired import JointOutcomes
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator, retirement_age

    cfg = _config(retirement_years=3, num_simulations_main=8, current_age=40.0)
    sim = RetirementMonteCarloSimulator(cfg, main_seed_override=5)
    options = [{"rule": None}, {"rule": SYMMETRIC, "monthly_expenses": 2000.0}, {"rule": SpendingRule(*SYMMETRIC), "initial_balance": 5.0},
               {"rule": SYMMETRIC, "monthly_expenses": 2000.0}]
    years = {0: [[8, 0, 0, 0], [6, 0, 0, 0], [5, 0, 0, 0]], 1: [[8, 0, 0, 0], [8, 4, 0, 1], [7, 3, 2, 0]],
             2: [[8, 0, 0, 0], [4, 4, 4, 0], [3, 1, 1, 1]], 3: [[8, 0, 0, 0], [8, 4, 0, 1], [7, 3, 2, 0]]}
    successes = [5, 7, 2, 7]
    seen = []

    def fake_counts(working_months, records, n):
        seen.append((working_months, records, n))
        return np.array([[successes[k], n] + list(np.ravel(years[k])) for k in range(len(records))], dtype=np.int64)

    sim._rule_probe_counts = fake_counts
    doc = sim.compare_spending_rules(24, options)
    age = retirement_age(40.0, 24)
    assert seen == [(24, rule_options(cfg, options), 8)]
    assert doc["best"] == 1 and [r["probability"] for r in doc["options"]] == [62.5, 87.5, 25.0, 87.5]
    assert doc["options"][0]["rule"] is None and doc["options"][1]["rule"] == SpendingRule(*SYMMETRIC).as_dict()
    assert doc["options"][2]["initial_balance"] == 5.0 and doc["options"][1]["monthly_expenses"] == 2000.0
    assert doc["options"][0]["monthly_expenses"] == float(cfg.monthly_expenses)
    for k, row in enumerate(doc["options"]):
        assert row["years"] == SpendingRuleOutcomes(successes[k], 8, years[k], age).years()
        assert set(row) == {"initial_balance", "monthly_contribution", "monthly_expenses", "rule", "probability", "years"}
    assert set(doc) == {"options", "best"}
    # paired / outcomes: from the joint and per-option objects of the same options
    ok = np.array([[1, 1, 1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 0], [1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 0]], dtype=np.int64)
    joint = JointOutcomes(ok @ ok.T, 8, (2, 1))
    months = np.zeros((4, 37), dtype=np.int64)
    for k in range(4):
        months[k, 12 + k] = 8 - successes[k]
    per_option = OptionOutcomes(np.array(successes), 8, months, (0.05, 0.25, 0.5, 0.75, 0.95), np.arange(20.0).reshape(4, 5),
                                np.array(successes), age)
    calls = []
    sim.joint_outcomes_by_rules = lambda wm, opts, n=None: calls.append(("joint", wm, opts, n)) or joint
    sim.option_outcomes_by_rules = lambda wm, opts, n=None: calls.append(("outcomes", wm, opts, n)) or per_option
    full = sim.compare_spending_rules(24, options, 8, paired=True, outcomes=True)
    assert calls == [("joint", 24, options, 8), ("outcomes", 24, options, 8)]
    assert full["best"] == 1 and full["tied_with_best"] == joint.indistinguishable_from(1) and 3 in full["tied_with_best"]
    assert (full["all_succeed"], full["none_succeed"]) == (2, 1)
    for k, row in enumerate(full["options"]):
        assert row["vs_best"] == joint.difference(1, k)
        assert {f: row[f] for f in ("lasts_until_age", "median_ruin_age", "final_balance")} == per_option.row(k)
        assert {f: v for f, v in row.items() if f in doc["options"][k]} == doc["options"][k]
    only_paired = sim.compare_spending_rules(24, options, 8, paired=True)
    assert "vs_best" in only_paired["options"][0] and "final_balance" not in only_paired["options"][0] and "all_succeed" in only_paired
    only_outcomes = sim.compare_spending_rules(24, options, 8, outcomes=True)
    assert "vs_best" not in only_outcomes["options"][0] and "lasts_until_age" in only_outcomes["options"][0] and "all_succeed" not in only_outcomes
    with pytest.raises(ValueError, match="unknown key"):
        sim.compare_spending_rules(24, [{"rules": None}])


def test_levels_of_success_probability_with_rule_go_through_the_probe():
    """Two or more levels are ONE call of the rule probe's records (the config's other two amounts, the same rule); one level and
    none stay the plain rule launch."""
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = _config(num_simulations_main=200)
    sim = RetirementMonteCarloSimulator(cfg, main_seed_override=5)
    rule = SpendingRule(*SYMMETRIC)
    seen = []

    def fake_counts(working_months, records, n):
        seen.append((working_months, records, n))
        return np.array([[n - 10 * k, n] + [0] * (4 * 30) for k in range(len(records))], dtype=np.int64)

    sim._rule_probe_counts = fake_counts
    sim._rule_counts = lambda wm, rule_, params, n, multipliers=False: np.array([17, n] + [0] * 120, dtype=np.int64)
    got = sim.success_probability_with_rule(12, rule, [100.0, 200.0, 300.0])
    b0, c0 = float(cfg.initial_balance), float(cfg.monthly_contribution)
    assert seen == [(12, [(b0, c0, 100.0, rule), (b0, c0, 200.0, rule), (b0, c0, 300.0, rule)], 200)]
    assert isinstance(got, np.ndarray) and got.tolist() == [100.0, 95.0, 90.0]
    assert sim.success_probability_with_rule(12, rule, [100.0]).tolist() == [8.5] and sim.success_probability_with_rule(12, rule, 100.0) == 8.5
    assert sim.success_probability_with_rule(12, rule) == 8.5 and len(seen) == 1
