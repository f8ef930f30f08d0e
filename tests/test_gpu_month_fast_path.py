"""The wave-uniform fast month (csrc/mcr_device.h: WAVE-UNIFORM fix-ups; csrc/mcr_hip.hip: kFastMonth).  The tolerance month
tests its dust / empty fix-ups with one wave ballot and runs a straight-line body when no active lane qualifies.  The claim is
that this changes no bit: here the path kernel is compared with a build that always takes the lane-masked fix-ups
(-DMCR_K1_GENERAL_MONTH, loaded through MCR_HIP_LIBRARY in a child process), on scenarios that put fix-up lanes and ordinary
lanes in the same wave: tiny balances, allocations 0 and 1, paths that fail with a few dollars left, and the same with a
realized-gains rate near the closed form's limit.  Both builds are also held to the oracle at the suite's tolerance."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden
from monte_carlo_retirement_amd import Config, params_from_config
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY = ("start_balance", "final_balance", "years_to_ruin", "first_year_gross_withdrawal",
           "first_year_real_gross_withdrawal", "inflation_at_retirement", "success")
BINS = ("counters", "ruin_year_bins", "wr_obs_counts", "hist_bins")
SEED, N_PATHS, N_ORACLE = 777, 16384, 1024

# the child: one build of the library (MCR_HIP_LIBRARY, or the default one), per-path summaries and the count-only launch
CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E
spec = json.load(open(sys.argv[2]))
out = {}
for i, sc in enumerate(spec["scenarios"]):
    p = params_from_config(Config(**sc["cfg"]))
    r = E.run_batch_host(p, spec["seed"], 1, 0, spec["n"], sc["wm"], want_trajectories=False, hist_edges=spec["edges"])
    c = E.run_batch_host(p, spec["seed"], 1, 0, spec["n"], sc["wm"], want_summary=False, want_trajectories=False,
                         hist_edges=spec["edges"])
    for k, v in r.items():
        out[f"{i}/summary/{k}"] = np.asarray(v)
    for k, v in c.items():
        out[f"{i}/count/{k}"] = np.asarray(v)
np.savez(sys.argv[3], **out)
"""


def _scenarios():
    base = {g["name"]: g for g in load_golden("paths_injected.json")}["C1_config_json_wm233"]["cfg"]
    out = []
    for rate in (0.1, 0.999):
        taxed = dict(inv1_realized_gains_tax_rate=rate, inv2_realized_gains_tax_rate=rate,
                     inv1_use_realized_gains_tax_system=True, inv2_use_realized_gains_tax_system=True)
        # dollars and cents: balances cross the 1e-6 dust threshold inside the horizon (about a quarter of the paths fail)
        out.append((dict(base, **taxed, initial_balance=3.0, monthly_contribution=0.02, monthly_expenses=0.028,
                         retirement_years=12, other_income_streams=[]), 6))
        # allocation 0 and 1: one asset is empty and the drift is 0 every month
        for alloc in (0.0, 1.0):
            out.append((dict(base, **taxed, allocation_inv1_pct=alloc, retirement_years=25), 200))
        # a tenth of the paths fail, most of them with a few dollars left in their last month
        out.append((dict(base, **taxed, monthly_expenses=13000.0, retirement_years=25), 233))
    return out


@pytest.fixture(scope="module")
def general_month_library():
    from monte_carlo_retirement_amd.csrc import build as B

    return B.build(variant="general_month", extra_flags=["-DMCR_K1_GENERAL_MONTH"])


def _run_child(tmp_path, tag, lib, spec):
    spec_path, out = tmp_path / "spec.json", tmp_path / f"{tag}.npz"
    spec_path.write_text(json.dumps(spec))
    env = dict(os.environ)
    env.pop("MCR_HIP_LIBRARY", None)
    if lib:
        env["MCR_HIP_LIBRARY"] = lib
    subprocess.run([sys.executable, "-c", CHILD, REPO, str(spec_path), str(out)], env=env, check=True, timeout=600)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_fast_month_bit_identical_to_general_month(tmp_path, general_month_library):
    scen = _scenarios()
    edges = [0.0, 1.0, 1e3, 1e5, 1e6, 1e7, 1e9]
    spec = {"seed": SEED, "n": N_PATHS, "edges": edges, "scenarios": [{"cfg": c, "wm": wm} for c, wm in scen]}
    fast = _run_child(tmp_path, "fast", None, spec)
    general = _run_child(tmp_path, "general", general_month_library, spec)
    assert sorted(fast) == sorted(general)
    for i, (cfg, wm) in enumerate(scen):
        for k in SUMMARY + BINS:
            got, exp = fast[f"{i}/summary/{k}"], general[f"{i}/summary/{k}"]
            assert got.tobytes() == exp.tobytes(), f"scenario {i} ({cfg['allocation_inv1_pct']=}, wm={wm}): {k} differs"
        for k in BINS:
            got, exp = fast[f"{i}/count/{k}"], general[f"{i}/count/{k}"]
            assert np.array_equal(got, exp), f"scenario {i}: count-only {k} differs"
    # the scenarios do exercise both sides: some paths fail, some succeed
    fails = sum(int(fast[f"{i}/summary/counters"][1] - fast[f"{i}/summary/counters"][0]) for i in range(len(scen)))
    assert 0 < fails < len(scen) * N_PATHS


def test_fast_month_within_tolerance_of_oracle(tmp_path):
    scen = _scenarios()
    spec = {"seed": SEED, "n": N_ORACLE, "edges": [0.0, 1e9], "scenarios": [{"cfg": c, "wm": wm} for c, wm in scen]}
    gpu = _run_child(tmp_path, "fast", None, spec)
    for i, (cfg, wm) in enumerate(scen):
        cpu = O.run_batch(params_from_config(Config(**cfg)), SEED, 1, 0, N_ORACLE, wm, want_trajectories=False)
        assert np.array_equal(gpu[f"{i}/summary/success"], cpu["success"]), f"scenario {i}: Success flags differ"
        assert gpu[f"{i}/summary/counters"].tolist() == cpu["counters"].tolist()
        # 1e-9 relative to the larger of the value and the PATH'S money scale (its balance at retirement), + 1e-6: the
        # suite's convention (test_gpu_parity.py) — a final balance can be a small remainder of a large path
        scale = np.maximum(np.abs(cpu["start_balance"]), 1.0)
        for k in SUMMARY:
            got, exp = gpu[f"{i}/summary/{k}"].astype(np.float64), cpu[k].astype(np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(exp)), f"scenario {i}: {k} NaN pattern differs"
            err = np.abs(np.nan_to_num(got) - np.nan_to_num(exp))
            assert np.all(err <= 1e-6 + 1e-9 * np.maximum(np.abs(np.nan_to_num(exp)), scale)), (i, k, float(err.max()))
