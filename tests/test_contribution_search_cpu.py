"""The minimum-contribution search (monte_carlo_retirement_amd/saving.py) against stub probes, its multi-rank form through
`distributed.probe_candidates`, the CLI's argument checks, and the new C entry point's behaviour without a GPU."""

from __future__ import annotations

import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.saving import CONTRIBUTION_CAP, search_minimum_contribution


class Stub:
    """probe_levels(levels) -> [%] from a function of the level; records the calls."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, levels):
        self.calls.append(list(levels))
        return [self.fn(x) for x in levels]


def step(threshold):
    return lambda x: 90.0 if x >= threshold else 10.0


@pytest.mark.parametrize("threshold,start", [(3456.78, 1000.0), (1.0, 1.0), (0.37, 5.0), (987654.32, 0.0), (2500.0, 2500.0)])
@pytest.mark.parametrize("L", [1, 2, 8, 15])
def test_monotone_step_is_found_to_the_resolution(threshold, start, L):
    probe = Stub(step(threshold))
    x, p, curve = search_minimum_contribution(probe, 85.0, start, levels_per_call=L, resolution=1.0)
    assert x - 1.0 - 1e-9 < threshold <= x
    assert p == 90.0
    assert all(len(c) <= L for c in probe.calls)
    # the next evaluated level below x misses, and is within the resolution
    below = max(c["monthly_contribution"] for c in curve if c["monthly_contribution"] < x)
    assert x - below <= 1.0 + 1e-9 and probe.fn(below) < 85.0


@pytest.mark.parametrize("threshold", [0.01, 12.34, 1234.56, 98765.43])
def test_step_gives_the_exact_cent(threshold):
    x, p, _ = search_minimum_contribution(Stub(step(threshold)), 85.0, 100.0, levels_per_call=15, resolution=0.01)
    assert x == threshold and p == 90.0


def test_probe_count_bound():
    for L in (1, 2, 4, 8, 15):
        for threshold in (0.5, 77.7, 5000.0, 123456.78):
            probe = Stub(step(threshold))
            search_minimum_contribution(probe, 85.0, 100.0, levels_per_call=L, resolution=1.0)
            # bracket calls: the ladder up to the first hit; then the refinement of (lo, hi)
            rungs = [0.0] + [100.0 * 2 ** k for k in range(40)]
            first_hit = next(i for i, r in enumerate(rungs) if r >= threshold)
            bracket = math.ceil((first_hit + 1) / L)
            lo, hi = rungs[first_hit - 1], rungs[first_hit]
            refine = math.ceil(math.log(max(hi - lo, 1.0) / 1.0) / math.log(L + 1) - 1e-12)
            assert len(probe.calls) <= bracket + refine, (L, threshold, probe.calls)


@pytest.mark.parametrize("seed", range(6))
def test_noisy_non_monotone_keeps_the_invariant(seed):
    rng = np.random.default_rng(seed)
    noise = {}

    def fn(x):   # rising curve with large, deterministic per-level noise: many local reversals
        if x not in noise:
            noise[x] = rng.normal(0.0, 4.0)
        return float(np.clip(20.0 + x / 50.0 + noise[x], 0.0, 100.0))

    probe = Stub(fn)
    target = 80.0
    x, p, curve = search_minimum_contribution(probe, target, 100.0, levels_per_call=8, resolution=0.5)
    seen = {c["monthly_contribution"]: c["probability"] for c in curve}
    assert seen[x] == p >= target
    lo = max(v for v in seen if v < x)
    assert seen[lo] < target and x - lo <= 0.5 + 1e-9
    assert len(seen) == len(curve)   # every level evaluated once


def test_no_contribution_needed_returns_zero():
    probe = Stub(lambda x: 95.0)
    x, p, curve = search_minimum_contribution(probe, 85.0, 2000.0, levels_per_call=15)
    assert (x, p) == (0.0, 95.0)
    assert len(probe.calls) == 1 and probe.calls[0][0] == 0.0 and curve[0] == {"monthly_contribution": 0.0, "probability": 95.0}


def test_never_reaching_returns_minus_one_and_warns():
    probe = Stub(lambda x: 10.0 + x * 1e-7)
    with pytest.warns(RuntimeWarning, match="cap"):
        x, p, curve = search_minimum_contribution(probe, 85.0, 3000.0, levels_per_call=15)
    assert x == -1.0 and p == probe.fn(CONTRIBUTION_CAP)
    assert max(c["monthly_contribution"] for c in curve) == CONTRIBUTION_CAP


def test_levels_are_whole_cents_and_curve_and_events_have_their_shape():
    events = []
    probe = Stub(step(1234.567))
    x, p, curve = search_minimum_contribution(probe, 85.0, 333.333, levels_per_call=4, resolution=0.01, on_level=events.append)
    for call in probe.calls:
        for v in call:
            assert v == round(v, 2)
    assert x == 1234.57
    assert [c["monthly_contribution"] for c in curve] == [v for call in probe.calls for v in call]
    assert all(set(c) == {"monthly_contribution", "probability"} for c in curve)
    assert len(events) == len(curve)
    assert {e["type"] for e in events} == {"contribution_search_iter"}
    assert all(set(e) == {"type", "iteration", "monthly_contribution", "probability", "target", "lo", "hi"} for e in events)
    assert [e["iteration"] for e in events] == [i + 1 for i, call in enumerate(probe.calls) for _ in call]
    assert [e["monthly_contribution"] for e in events] == [c["monthly_contribution"] for c in curve]
    assert all(e["target"] == 85.0 for e in events)
    assert curve[0]["monthly_contribution"] == 0.0 and curve[1]["monthly_contribution"] == 333.33


def test_deterministic():
    runs = [search_minimum_contribution(Stub(lambda x: (x * 7919 % 97) / 3.0 + x / 40.0), 75.0, 50.0) for _ in range(2)]
    assert runs[0] == runs[1]


def test_argument_checks():
    with pytest.raises(ValueError):
        search_minimum_contribution(Stub(step(1.0)), 85.0, 1.0, levels_per_call=0)
    with pytest.raises(ValueError):
        search_minimum_contribution(Stub(step(1.0)), 85.0, 1.0, resolution=0.0)
    with pytest.raises(ValueError):
        search_minimum_contribution(Stub(step(1.0)), 85.0, 1.0, resolution=-1.0)


_WORKER = r"""
import json, sys
sys.path.insert(0, {repo!r})
import torch.distributed as dist
from monte_carlo_retirement_amd import distributed as D
from monte_carlo_retirement_amd.saving import search_minimum_contribution
dist.init_process_group("gloo")
rank = dist.get_rank()
n_total, shard_min = int(sys.argv[1]), int(sys.argv[2])
calls = []

def level_pct(x):   # a success % that every rank can reconstruct from integer counts
    return 20.0 + (int(x * 100) * 7919 % 1009) / 200.0 + x / 30.0

def probe_levels(levels):
    def probe(path_begin, count, idx):
        calls.append((path_begin, count, list(idx)))
        out = []
        for i in idx:   # successes of paths [path_begin, path_begin + count) at level i: a deterministic share
            share = max(0.0, min(1.0, level_pct(levels[i]) / 100.0))
            out.append([int(round(share * (path_begin + count))) - int(round(share * path_begin)), count])
        return out
    counts = D.probe_candidates(list(range(len(levels))), n_total, shard_min, probe)
    return [float(counts[i, 0]) / n_total * 100.0 for i in range(len(levels))]

res = search_minimum_contribution(probe_levels, 80.0, 100.0, levels_per_call=15, resolution=1.0)
json.dump({{"res": res, "calls": calls}}, open(sys.argv[3] + str(rank), "w"))
dist.destroy_process_group()
"""


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("n_total,shard_min", [(1000, 10**6), (100_003, 1000)])   # split by level / sharded by path range
def test_two_ranks_return_identical_results(tmp_path, n_total, shard_min):
    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                   LOCAL_RANK=str(rank), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c",
                                       _WORKER.format(repo=REPO), str(n_total), str(shard_min), out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        o, _ = p.communicate(timeout=300)
        assert p.returncode == 0, o.decode()[-3000:]
    r0, r1 = (json.load(open(out + str(r))) for r in range(2))
    assert r0["res"] == r1["res"]
    x, p, curve = r0["res"]
    assert x > 0 and p >= 80.0
    lo = max(c["monthly_contribution"] for c in curve if c["monthly_contribution"] < x)
    assert next(c["probability"] for c in curve if c["monthly_contribution"] == lo) < 80.0
    if n_total >= shard_min:   # every rank probed every level on its own path shard
        assert {c[0] for c in r0["calls"]} == {0} and {c[0] for c in r1["calls"]} == {(n_total + 1) // 2}
    else:                      # levels split across the ranks, whole path range each
        idx0 = [i for c in r0["calls"] for i in c[2]]
        idx1 = [i for c in r1["calls"] for i in c[2]]
        assert all(i % 2 == 0 for i in idx0) and all(i % 2 == 1 for i in idx1)


def test_entry_point_is_exported_and_declared():
    assert "mcr_probe_contributions_rng" in N.ABI_SYMBOLS
    assert N.MCR_ABI_VERSION == 8
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert "int mcr_probe_contributions_rng(" in header and "const double* monthly_contributions" in header


def test_cli_min_contribution_needs_working_months():
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--min-contribution"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--working-months" in r.stderr and not r.stdout.strip()


def test_fails_loudly_without_a_gpu():
    """In a child process (a HIP runtime initialised here would stay open for the session): without a device the call
    returns MCR_ERR_NO_DEVICE and the Python wrapper raises; it never computes on the CPU."""
    code = (
        "import ctypes as C, json\n"
        "from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config\n"
        "from monte_carlo_retirement_amd import _native as N, engine as E\n"
        "lib = N.load_library()\n"
        "if lib.mcr_device_count() > 0:\n"
        "    print(json.dumps({'gpu': True})); raise SystemExit(0)\n"
        "p = params_from_config(Config(**load_config_from_json('scenarios/config.json')))\n"
        "lv = (C.c_double * 2)(100.0, 200.0)\n"
        "rng = N.McrRng(); rng.kind = N.MCR_RNG_PHILOX; rng.philox_seed = 1\n"
        "rc = lib.mcr_probe_contributions_rng(C.byref(p), C.byref(rng), 0, 0, 64, 12, lv, 2, None, 0, None)\n"
        "msg = N.last_error()\n"
        "try:\n"
        "    E.probe_contributions(p, 1, 0, 0, 64, 12, [100.0, 200.0]); raised = ''\n"
        "except RuntimeError as e:\n"
        "    raised = str(e)\n"
        "print(json.dumps({'gpu': False, 'rc': rc, 'msg': msg, 'raised': raised}))\n"
    )
    lib_so = os.path.join(REPO, "monte_carlo_retirement_amd", "csrc", "libmcr_hip.so")
    if not os.path.exists(lib_so):
        from monte_carlo_retirement_amd.csrc import build

        build.build()
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if out["gpu"]:
        pytest.skip("a GPU is present")
    assert out["rc"] == -2 and "no usable HIP device" in out["msg"]
    assert out["raised"]
