"""The lockstep maximum-spending search (`spending.search_maximum_expenses_many`) against the single search on stub probes,
the grid probe's entry point without a GPU, and the grid's multi-rank form through `distributed.probe_candidates`."""

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
from monte_carlo_retirement_amd.spending import EXPENSE_CAP, search_maximum_expenses, search_maximum_expenses_many


def step(threshold):
    return lambda x: 90.0 if x <= threshold else 10.0


def noisy(seed):
    rng = np.random.default_rng(seed)
    noise = {}

    def fn(x):
        if x not in noise:
            noise[x] = rng.normal(0.0, 4.0)
        return float(np.clip(100.0 - x / 50.0 + noise[x], 0.0, 100.0))
    return fn


class Rows:
    """probe_rows(rows, levels_2d) from one function of the level per search; records every call."""

    def __init__(self, fns):
        self.fns, self.calls = fns, []

    def __call__(self, rows, levels_2d):
        assert len({len(r) for r in levels_2d}) == 1          # rectangular
        self.calls.append((list(rows), [list(r) for r in levels_2d]))
        return [[self.fns[i](x) for x in row] for i, row in zip(rows, levels_2d)]


def _singles(fns, target, starts, **kw):
    out = []
    for i, (fn, s) in enumerate(zip(fns, starts)):
        events = []
        calls = []

        def probe(levels, fn=fn):
            calls.append(list(levels))
            return [fn(x) for x in levels]
        res = search_maximum_expenses(probe, target, s, on_level=events.append, **kw)
        out.append((res, events, calls))
    return out


CASES = {
    "steps": ([step(3456.78), step(1.0), step(987654.32), step(0.37), step(2500.0)], [1000.0, 1.0, 0.0, 5.0, 2500.0], 85.0),
    "noisy": ([noisy(s) for s in range(4)], [100.0, 300.0, 1.0, 5000.0], 80.0),
    "zero_misses": ([lambda x: 40.0, step(777.0), lambda x: 84.99], [2000.0, 50.0, 1.0], 85.0),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("L", [1, 4, 15])
def test_lockstep_equals_sequential_searches(case, L):
    fns, starts, target = CASES[case]
    months = [120 + 12 * i for i in range(len(fns))]
    kw = dict(levels_per_call=L, resolution=0.5 if case == "noisy" else 1.0)
    events = []
    probe = Rows(fns)
    many = search_maximum_expenses_many(probe, target, starts, on_level=events.append, working_months=months, **kw)
    singles = _singles(fns, target, starts, **kw)
    for i, (res, ev, calls) in enumerate(singles):
        assert many[i] == res, i
        mine = [e for e in events if e["working_months"] == months[i]]
        assert [{k: v for k, v in e.items() if k != "working_months"} for e in mine] == ev
        # the calls of search i: its rows of the lockstep calls, without the padding
        lock = [levels[rows.index(i)][: len(calls[k])] for k, (rows, levels) in enumerate(c for c in probe.calls if i in c[0])]
        assert lock == calls
    # one lockstep call per round: as many as the longest single search made, every width within the per-call limit
    assert len(probe.calls) == max(len(c) for _, _, c in singles)
    assert all(len(levels[0]) <= L for _, levels in probe.calls)
    # finished searches drop out
    assert all(len(rows) == len(set(rows)) for rows, _ in probe.calls)
    assert [len(rows) for rows, _ in probe.calls] == sorted((len(rows) for rows, _ in probe.calls), reverse=True)


def test_cap_reached():
    fns = [lambda x: 100.0, step(5000.0)]
    probe = Rows(fns)
    with pytest.warns(RuntimeWarning, match="cap"):
        many = search_maximum_expenses_many(probe, 85.0, [3000.0, 3000.0], levels_per_call=15)
    with pytest.warns(RuntimeWarning, match="cap"):
        want = search_maximum_expenses(lambda lv: [100.0] * len(lv), 85.0, 3000.0, levels_per_call=15)
    assert many[0] == want and many[0][0] == EXPENSE_CAP
    assert many[1] == search_maximum_expenses(lambda lv: [step(5000.0)(x) for x in lv], 85.0, 3000.0, levels_per_call=15)


def test_padding_does_not_leak():
    """A search with fewer levels in a round gets its own last level repeated; those results never reach its curve or
    events (a stub that answers padded positions with garbage proves it)."""
    fns = [step(1234.56), step(98765.43)]

    def probe_rows(rows, levels_2d):
        out = []
        for i, row in zip(rows, levels_2d):
            seen, vals = set(), []
            for x in row:
                vals.append(-1.0 if x in seen else fns[i](x))   # a repeated (padded) level answers -1
                seen.add(x)
            out.append(vals)
        return out

    events = []
    many = search_maximum_expenses_many(probe_rows, 85.0, [10.0, 10.0], levels_per_call=6, on_level=events.append)
    for (x, p, curve), fn in zip(many, fns):
        assert all(c["probability"] in (90.0, 10.0) for c in curve)
        assert len({c["monthly_expenses"] for c in curve}) == len(curve)
    assert all(e["probability"] in (90.0, 10.0) for e in events)
    assert [m[0] for m in many] == [search_maximum_expenses(lambda lv, f=f: [f(x) for x in lv], 85.0, 10.0, levels_per_call=6)[0]
                                    for f in fns]


def test_argument_checks():
    probe = Rows([step(1.0)])
    with pytest.raises(ValueError):
        search_maximum_expenses_many(probe, 85.0, [1.0], levels_per_call=0)
    with pytest.raises(ValueError):
        search_maximum_expenses_many(probe, 85.0, [1.0], resolution=0.0)
    with pytest.raises(ValueError):
        search_maximum_expenses_many(probe, 85.0, [1.0], working_months=[1, 2])
    with pytest.raises(RuntimeError):
        search_maximum_expenses_many(lambda rows, lv: [[50.0] * len(lv[0])], 85.0, [1.0, 2.0])
    with pytest.raises(RuntimeError):
        search_maximum_expenses_many(lambda rows, lv: [[50.0] for _ in rows], 85.0, [1.0, 2.0], levels_per_call=4)
    assert search_maximum_expenses_many(probe, 85.0, []) == []
    assert probe.calls == []


def test_entry_point_is_declared_and_exported():
    assert "mcr_probe_grid_rng" in N.ABI_SYMBOLS
    assert N.MCR_ABI_VERSION == 8
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert "int mcr_probe_grid_rng(" in header and "#define MCR_ABI_VERSION 8" in header


def test_fails_loudly_without_a_gpu():
    """In a child process: without a device the call returns MCR_ERR_NO_DEVICE and the Python wrapper raises; it never
    computes on the CPU."""
    code = (
        "import ctypes as C, json\n"
        "from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config\n"
        "from monte_carlo_retirement_amd import _native as N, engine as E\n"
        "lib = N.load_library()\n"
        "if lib.mcr_device_count() > 0:\n"
        "    print(json.dumps({'gpu': True})); raise SystemExit(0)\n"
        "p = params_from_config(Config(**load_config_from_json('scenarios/config.json')))\n"
        "m = (C.c_int32 * 2)(12, 24)\n"
        "lv = (C.c_double * 4)(1000.0, 2000.0, 1500.0, 2500.0)\n"
        "rng = N.McrRng(); rng.kind = N.MCR_RNG_PHILOX; rng.philox_seed = 1\n"
        "rc = lib.mcr_probe_grid_rng(C.byref(p), C.byref(rng), 0, 0, 64, m, 2, lv, 2, None, 0, None)\n"
        "msg = N.last_error()\n"
        "try:\n"
        "    E.probe_grid(p, 1, 0, 0, 64, [12, 24], [[1000.0, 2000.0], [1500.0, 2500.0]]); raised = ''\n"
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


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("n_total,shard_min", [(1000, 10**6), (100_003, 1000)])   # split by row / sharded by path range
def test_two_ranks_return_identical_matrices(tmp_path, n_total, shard_min):
    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                   LOCAL_RANK=str(rank), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                       os.path.join(REPO, "tests", "grid_dist_worker.py"), str(n_total), str(shard_min), out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        o, _ = p.communicate(timeout=300)
        assert p.returncode == 0, o.decode()[-3000:]
    r0, r1 = (json.load(open(out + str(r))) for r in range(2))
    assert r0["grid"] == r1["grid"] and r0["frontier"] == r1["frontier"]
    grid = np.array(r0["grid"])
    months, levels = r0["months"], r0["levels"]
    assert grid.shape == (len(months), len(levels), 2)
    # every cell is the whole range's count, whichever rank computed it
    for c, m in enumerate(months):
        for k, x in enumerate(levels):
            share = r0["share"][c][k]
            assert grid[c, k].tolist() == [int(round(share * n_total)), n_total]
    for (x, p, curve), m in zip(r0["frontier"], months):
        assert p >= 80.0 and any(c["monthly_expenses"] == x for c in curve)
    if n_total >= shard_min:   # every rank probed every row on its own path shard
        assert {c[0] for c in r0["calls"]} == {0} and {c[0] for c in r1["calls"]} == {(n_total + 1) // 2}
    else:                      # rows split across the ranks, whole path range each
        assert all(i % 2 == 0 for c in r0["calls"] for i in c[2]) and all(i % 2 == 1 for c in r1["calls"] for i in c[2])
    assert math.isfinite(r0["frontier"][0][1])
