"""The required-income search and the option records (monte_carlo_retirement_amd/income.py) against stub probes, the search
generator it shares with `nestegg` (whose results and events must be what they were), and the income probe's C entry points:
declaration, binding, struct layout, and a loud failure without a GPU."""

from __future__ import annotations

import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, load_config_from_json
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.income import (INCOME_AMOUNT_CAP, INCOME_OPTION_FIELDS, income_options,
                                               search_minimum_income_amount, stream_index)
from monte_carlo_retirement_amd.nestegg import search_minimum_initial_balance
from monte_carlo_retirement_amd.saving import CONTRIBUTION_CAP, search_minimum_contribution

KEY = "monthly_amount_today"


class Stub:
    """probe_levels(levels) -> [%] from a function of the level; records the calls."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, levels):
        self.calls.append(list(levels))
        return [self.fn(x) for x in levels]


def step(threshold):
    return lambda x: 90.0 if x >= threshold else 10.0


def _noisy(seed):
    rng = np.random.default_rng(seed)
    noise = {}

    def fn(x):   # rising curve with large, deterministic per-level noise: many local reversals
        if x not in noise:
            noise[x] = rng.normal(0.0, 4.0)
        return float(np.clip(20.0 + x / 50.0 + noise[x], 0.0, 100.0))

    return fn


@pytest.mark.parametrize("threshold,start", [(3456.78, 1000.0), (1.0, 1.0), (0.37, 5.0), (987654.3, 0.0), (2500.0, 2500.0)])
@pytest.mark.parametrize("L", [1, 2, 8, 15])
def test_monotone_step_is_found_to_the_resolution(threshold, start, L):
    probe = Stub(step(threshold))
    x, p, curve = search_minimum_income_amount(probe, 85.0, start, levels_per_call=L, resolution=1.0)
    assert x - 1.0 - 1e-9 < threshold <= x
    assert p == 90.0 and x == round(x, 2)
    assert all(len(c) <= L for c in probe.calls)
    seen = {c[KEY]: c["probability"] for c in curve}
    lo = max(v for v in seen if v < x)
    assert x - lo <= 1.0 + 1e-9 and seen[x] >= 85.0 > seen[lo]


@pytest.mark.parametrize("threshold", [0.01, 12.34, 1234.56, 98765.43])
def test_step_gives_the_exact_cent(threshold):
    x, p, _ = search_minimum_income_amount(Stub(step(threshold)), 85.0, 1000.0, levels_per_call=15, resolution=0.01)
    assert x == threshold and p == 90.0


@pytest.mark.parametrize("seed", range(6))
def test_noisy_non_monotone_keeps_the_invariant(seed):
    probe = Stub(_noisy(seed))
    target = 80.0
    x, p, curve = search_minimum_income_amount(probe, target, 100.0, levels_per_call=8, resolution=0.5)
    seen = {c[KEY]: c["probability"] for c in curve}
    assert seen[x] == p >= target
    lo = max(v for v in seen if v < x)
    assert seen[lo] < target and x - lo <= 0.5 + 1e-9
    assert len(seen) == len(curve)   # every level evaluated once


def test_probe_count_bound():
    """bracket + ceil(log_{L+1}(range / resolution)) calls"""
    for L in (1, 2, 4, 8, 15):
        for threshold in (0.5, 77.7, 5000.0, 1234567.8):
            probe = Stub(step(threshold))
            search_minimum_income_amount(probe, 85.0, 1000.0, levels_per_call=L, resolution=1.0)
            rungs = [0.0] + [1000.0 * 2 ** k for k in range(40)]
            first_hit = next(i for i, r in enumerate(rungs) if r >= threshold)
            bracket = math.ceil((first_hit + 1) / L)
            lo, hi = rungs[first_hit - 1], rungs[first_hit]
            refine = math.ceil(math.log(max(hi - lo, 1.0) / 1.0) / math.log(L + 1) - 1e-12)
            assert len(probe.calls) <= bracket + refine, (L, threshold, probe.calls)


def test_target_met_at_zero_returns_zero():
    probe = Stub(lambda x: 95.0)
    x, p, curve = search_minimum_income_amount(probe, 85.0, 2000.0, levels_per_call=15)
    assert (x, p) == (0.0, 95.0)
    assert len(probe.calls) == 1 and probe.calls[0][0] == 0.0 and curve[0] == {KEY: 0.0, "probability": 95.0}


def test_never_reaching_returns_minus_one_and_warns():
    probe = Stub(lambda x: 10.0 + x * 1e-10)
    with pytest.warns(RuntimeWarning, match="cap"):
        x, p, curve = search_minimum_income_amount(probe, 85.0, 3000.0, levels_per_call=15)
    assert INCOME_AMOUNT_CAP == 1e8 == CONTRIBUTION_CAP
    assert x == -1.0 and p == probe.fn(INCOME_AMOUNT_CAP)
    assert max(c[KEY] for c in curve) == INCOME_AMOUNT_CAP


def test_levels_are_whole_cents_and_curve_and_events_have_their_shape():
    events = []
    probe = Stub(step(1234.567))
    x, p, curve = search_minimum_income_amount(probe, 85.0, 333.333, levels_per_call=4, resolution=0.01, on_level=events.append)
    assert all(v == round(v, 2) for call in probe.calls for v in call)
    assert x == 1234.57
    assert [c[KEY] for c in curve] == [v for call in probe.calls for v in call]
    assert all(set(c) == {KEY, "probability"} for c in curve)
    assert len(events) == len(curve)
    assert {e["type"] for e in events} == {"income_amount_search_iter"}
    assert all(set(e) == {"type", "iteration", KEY, "probability", "target", "lo", "hi"} for e in events)
    assert [e["iteration"] for e in events] == [i + 1 for i, call in enumerate(probe.calls) for _ in call]
    assert [e[KEY] for e in events] == [c[KEY] for c in curve]
    assert curve[0][KEY] == 0.0 and curve[1][KEY] == 333.33
    # the bracket's events carry no bounds, the refinement's carry the bracket P(hi) >= target > P(lo) found so far
    refine = [e for e in events if e["lo"] is not None]
    assert refine and all(e["lo"] < e["hi"] for e in refine)
    assert all(e["hi"] is None for e in events if e["lo"] is None)


def test_argument_checks():
    for kw in ({"levels_per_call": 0}, {"resolution": 0.0}, {"resolution": -1.0}):
        with pytest.raises(ValueError):
            search_minimum_income_amount(Stub(step(1.0)), 85.0, 1.0, **kw)
    with pytest.raises(RuntimeError, match="returned"):
        search_minimum_income_amount(lambda levels: [], 85.0, 1.0)


# ---- the generator is nestegg's, parameterised: its own search, and saving's restatement of it, are what they were ---------
def _rename(rows, old, new, old_type=None, new_type=None):
    out = []
    for r in rows:
        r = {(new if k == old else k): v for k, v in r.items()}
        if old_type is not None and r.get("type") == old_type:
            r["type"] = new_type
        out.append(r)
    return out


@pytest.mark.parametrize("fn,start,L,res", [(step(345.67), 1.0, 7, 1.0), (step(8_765_432.1), 1000.0, 15, 0.01), (_noisy(3), 100.0, 8, 0.5),
                                            (lambda x: 95.0, 50.0, 3, 1.0), (step(0.02), 250.0, 1, 1.0)])
def test_the_three_searches_walk_the_same_levels(fn, start, L, res):
    """One procedure, three names: the balance search (the generator's defaults) and the contribution search (its
    restatement in saving.py) give the levels, results and events they gave before the generator took a key, and the income
    search gives the same under its own key and event name."""
    runs = {}
    for name, search, key, ev_type in (("income", search_minimum_income_amount, KEY, "income_amount_search_iter"),
                                       ("balance", search_minimum_initial_balance, "initial_balance", "initial_balance_search_iter"),
                                       ("saving", search_minimum_contribution, "monthly_contribution", "contribution_search_iter")):
        probe, events = Stub(fn), []
        x, p, curve = search(probe, 80.0, start, levels_per_call=L, resolution=res, cap=1e8, on_level=events.append)
        assert all(set(c) == {key, "probability"} for c in curve)
        assert {e["type"] for e in events} == {ev_type}
        assert all(set(e) == {"type", "iteration", key, "probability", "target", "lo", "hi"} for e in events)
        runs[name] = (x, p, _rename(curve, key, "level"), _rename(events, key, "level", ev_type, "iter"), probe.calls)
    assert runs["income"] == runs["balance"] == runs["saving"]


def test_balance_search_events_and_warning_are_unchanged():
    """The literal shape of an event and of the cap warning of `nestegg.search_minimum_initial_balance`, as they were."""
    events = []
    x, p, curve = search_minimum_initial_balance(Stub(step(3.0)), 85.0, 2.0, levels_per_call=2, resolution=1.0, on_level=events.append)
    assert (x, p) == (3.0, 90.0)
    assert curve == [{"initial_balance": 0.0, "probability": 10.0}, {"initial_balance": 2.0, "probability": 10.0},
                     {"initial_balance": 4.0, "probability": 90.0}, {"initial_balance": 8.0, "probability": 90.0},
                     {"initial_balance": 3.0, "probability": 90.0}]
    assert events[0] == {"type": "initial_balance_search_iter", "iteration": 1, "initial_balance": 0.0, "probability": 10.0,
                         "target": 85.0, "lo": None, "hi": None}
    assert events[-1] == {"type": "initial_balance_search_iter", "iteration": 3, "initial_balance": 3.0, "probability": 90.0,
                          "target": 85.0, "lo": 2.0, "hi": 4.0}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert search_minimum_initial_balance(Stub(lambda x: 1.0), 85.0, 1e10, cap=1e11)[0] == -1.0
    assert [str(x.message) for x in w] == ["required-starting-balance search reached the cap of 1e+11 without reaching the target"]
    with pytest.warns(RuntimeWarning, match=r"^required-income search reached the cap of 1e\+08 without reaching the target$"):
        search_minimum_income_amount(Stub(lambda x: 1.0), 85.0, 1e7)


# ---- option records ---------------------------------------------------------------------------------------------------------
def _config(**over):
    d = load_config_from_json(os.path.join(REPO, "scenarios", "config.json"))
    d.update(over)
    return Config(**d)


def test_income_options_fill_defaults_and_find_the_stream():
    cfg = _config()
    assert INCOME_OPTION_FIELDS == ("initial_balance", "monthly_contribution", "monthly_expenses", "monthly_amount_today",
                                    "start_at_age", "duration_years")
    triple = (cfg.initial_balance, cfg.monthly_contribution, cfg.monthly_expenses)
    # stream 0 by index and by name: 4000 a month from 65 for life
    own0 = triple + (4000.0, 65.0, None)
    assert income_options(cfg, 0, [{}]) == [own0] == income_options(cfg, "State Pension", [{}])
    # stream 1: 0 a month from 40 for 35 years
    assert income_options(cfg, 1, [{}]) == [triple + (0.0, 40.0, 35)] == income_options(cfg, "Rental Income (Apt)", [{}])
    got = income_options(cfg, "State Pension", [
        {"start_at_age": 62, "monthly_amount_today": 2800}, {"duration_years": 0}, {"duration_years": None},
        {"initial_balance": 1.5, "monthly_contribution": 2, "monthly_expenses": 3, "monthly_amount_today": 4, "start_at_age": 5,
         "duration_years": 6}])
    assert got == [triple + (2800.0, 62.0, None), triple + (4000.0, 65.0, 0), own0, (1.5, 2.0, 3.0, 4.0, 5.0, 6)]
    assert all(isinstance(x, float) for r in got for x in r[:5])
    assert income_options(cfg, 1, [{"duration_years": None}])[0][5] is None     # None replaces the stream's own 35
    assert income_options(cfg, 0, []) == []
    assert stream_index(cfg, 1) == 1 == stream_index(cfg, "Rental Income (Apt)")


def test_income_options_reject_unknown_keys_and_streams():
    cfg = _config()
    with pytest.raises(ValueError, match=r"options\[1\].*tax_rate"):
        income_options(cfg, 0, [{}, {"tax_rate": 0.5}])
    with pytest.raises(ValueError, match="inflation_indexed"):
        income_options(cfg, 0, [{"inflation_indexed": False}])
    with pytest.raises(ValueError, match="Annuity"):
        income_options(cfg, "Annuity", [{}])
    for bad in (2.5, -1, True):
        with pytest.raises(ValueError, match=r"options\[1\].*duration_years"):
            income_options(cfg, 0, [{}, {"duration_years": bad}])
    assert income_options(cfg, 0, [{"duration_years": 3.0}])[0][5] == 3
    for bad in (2, -1, 0.5, True):
        with pytest.raises(ValueError):
            income_options(cfg, bad, [{}])
    streams = [dict(s.model_dump(), name="Pension") for s in cfg.other_income_streams]
    twins = _config(other_income_streams=streams)
    with pytest.raises(ValueError, match=r"ambiguous.*\[0, 1\]"):
        income_options(twins, "Pension", [{}])
    assert income_options(twins, 1, [{}])[0][3:] == (0.0, 40.0, 35)     # the index still works
    with pytest.raises(ValueError):
        income_options(_config(other_income_streams=[]), 0, [{}])


def test_simulator_rejects_bad_options_before_any_device_work():
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    class Double(RetirementMonteCarloSimulator):   # any step towards the device fails the test
        def _current_params(self):
            raise AssertionError("device work before the key check")

        _batch_rng = _local_device = _current_params

    sim = Double(_config())
    with pytest.raises(ValueError, match="tax_rate"):
        sim.success_probability_by_income_options(0, 0, [{"start_at_age": 62.0}, {"tax_rate": 0.1}], 100)
    with pytest.raises(ValueError, match="Annuity"):
        sim.compare_claiming_options(0, "Annuity", [{}], 100)
    with pytest.raises(ValueError, match="Annuity"):
        sim.find_minimum_income_amount(0, "Annuity", verbose=False)
    assert sim.success_probability_by_income_options(0, "State Pension", [], 100).shape == (0,)
    assert sim.compare_claiming_options(0, 0, [], 100) == {"stream": 0, "options": [], "best": None}


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_declared():
    for sym in ("mcr_probe_income_rng", "mcr_probe_income_last_fanout_launches"):
        assert sym in N.ABI_SYMBOLS
    assert N.MCR_ABI_VERSION == 8
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert re.search(r"#define\s+MCR_ABI_VERSION\s+8\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "int mcr_probe_income_rng(" in code and "const mcr_income_option* options" in code and "int32_t stream_index" in code
    assert "int mcr_probe_income_last_fanout_launches(void);" in code
    assert re.search(r"typedef struct mcr_income_option \{.*?\} mcr_income_option;", code, flags=re.S)
    assert C.sizeof(N.McrIncomeOption) == 48
    assert [f for f, _ in N.McrIncomeOption._fields_] == list(INCOME_OPTION_FIELDS) + ["reserved"]
    assert [t for _, t in N.McrIncomeOption._fields_] == [C.c_double] * 5 + [C.c_int32] * 2


def test_struct_layout_matches_what_a_c_compiler_sees(tmp_path):
    lines = ['printf("size %zu\\n", sizeof(mcr_income_option));']
    for fname, _ in N.McrIncomeOption._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(mcr_income_option, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    seen = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(seen["size"]) == 48 == C.sizeof(N.McrIncomeOption)
    for fname, _ in N.McrIncomeOption._fields_:
        assert int(seen[fname]) == getattr(N.McrIncomeOption, fname).offset, fname


def test_library_exports_the_entry_points_with_their_signatures():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    lib = N.load_library()
    assert hasattr(lib, "mcr_probe_income_rng") and hasattr(lib, "mcr_probe_income_last_fanout_launches")
    assert lib.mcr_probe_income_rng.argtypes[6] is C.c_int32
    assert lib.mcr_probe_income_rng.argtypes[7] == C.POINTER(N.McrIncomeOption)
    assert len(lib.mcr_probe_income_rng.argtypes) == 12
    assert lib.mcr_abi_version() == 8


def test_fails_loudly_without_a_gpu():
    """In a child process (a HIP runtime initialised here would stay open for the session): without a device the call
    returns MCR_ERR_NO_DEVICE — before it looks at its arguments, like the other probes — and the Python wrapper raises; it
    never computes on the CPU.  With a device present the GPU tests cover the call."""
    code = (
        "import ctypes as C, json\n"
        "from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config\n"
        "from monte_carlo_retirement_amd import _native as N, engine as E\n"
        "lib = N.load_library()\n"
        "if lib.mcr_device_count() > 0:\n"
        "    print(json.dumps({'gpu': True})); raise SystemExit(0)\n"
        "p = params_from_config(Config(**load_config_from_json('scenarios/config.json')))\n"
        "op = (N.McrIncomeOption * 2)(N.McrIncomeOption(1e5, 100.0, 3000.0, 2000.0, 62.0, -1, 0),\n"
        "                             N.McrIncomeOption(1e5, 100.0, 3000.0, 2500.0, 67.0, 10, 0))\n"
        "rng = N.McrRng(); rng.kind = N.MCR_RNG_PHILOX; rng.philox_seed = 1\n"
        "rc = lib.mcr_probe_income_rng(C.byref(p), C.byref(rng), 0, 0, 64, 12, 0, op, 2, None, 0, None)\n"
        "msg = N.last_error()\n"
        "launches = lib.mcr_probe_income_last_fanout_launches()\n"
        "try:\n"
        "    E.probe_income(p, 1, 0, 0, 64, 12, 0, [(1e5, 100.0, 3000.0, 2000.0, 62.0, None)] * 2); raised = ''\n"
        "except RuntimeError as e:\n"
        "    raised = str(e)\n"
        "print(json.dumps({'gpu': False, 'rc': rc, 'msg': msg, 'raised': raised, 'launches': launches}))\n"
    )
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if out["gpu"]:
        return
    assert out["rc"] == -2 and "no usable HIP device" in out["msg"]
    assert out["raised"] and out["launches"] == 0


def test_cli_rejects_option_lists_of_unequal_length():
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--income-options", "0", "--claim-ages", "62,67,70", "--claim-amounts", "1400,2000"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "equal lengths" in r.stderr and not r.stdout.strip()
