"""Grid probes (`mcr_probe_grid_rng`, `engine.probe_grid`), the success-probability grid and the max-spending frontier on the
GPU.

The contract: cell [c][k] equals, bit for bit, the counters of a count-only launch at working_months[c] with monthly_expenses =
levels[c][k] (`engine.probe_months` of a parameter block that differs only there) — on the grid fan-out route (Philox,
<= 16 streams, tolerance month, 2 .. 32 distinct months) and on the per-month route (NumPy stream, longer stream lists, the
exact month)."""

from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
from test_gpu_expense_probe import SCENARIOS, _cfg

pytestmark = pytest.mark.gpu
SEED = 0x6121_D00D
# unsorted, a repeat, 0, and months on both sides of config.json's stream that starts at age 65 (month 300 from age 40):
# the rows' parameter blocks differ in that stream's start month
MONTHS = [233, 0, 301, 37, 233, 299]


def _rows(base, months, L):
    """One level row per month: 0, 1e12 (every path fails), a repeat, and a spread that differs from row to row."""
    out = []
    for c, _ in enumerate(months):
        head = [base, 0.0, 1e12, base]
        spread = [round(base * (0.25 + 0.07 * k + 0.013 * c), 2) for k in range(max(0, L - len(head)))]
        out.append((head + spread)[:L])
    return out


def _per_cell(cfgd, seed, stream, begin, n, months, rows):
    out = []
    for wm, row in zip(months, rows):
        cells = []
        for x in row:
            q = params_from_config(Config(**dict(cfgd, monthly_expenses=x)))
            cells.append(E.probe_months(q, seed, stream, begin, n, [wm]).cpu().numpy()[0].tolist())
        out.append(cells)
    return out


def _check(cfgd, seed, n, begin, months, rows, stream=0):
    p = params_from_config(Config(**cfgd))
    got = E.probe_grid(p, seed, stream, begin, n, months, rows).cpu().numpy().tolist()
    want = _per_cell(cfgd, seed, stream, begin, n, months, rows)
    assert got == want, (months, n, begin, len(rows[0]))
    return got


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_cells_equal_plain_launches(name):
    cfgd = SCENARIOS[name]
    base = cfgd["monthly_expenses"]
    for months, L, n, begin in ((MONTHS, 17, 4097, 0), (MONTHS[:3], 4, 4097, 12_345), ([1, 360], 15, 63, 7)):
        got = _check(cfgd, SEED, n, begin, months, _rows(base, months, L))
        assert all(cell[1] == n for row in got for cell in row)
        assert all(row[2][0] == 0 for row in got)          # 1e12 a month fails everywhere
    assert got[0][1][0] > 0


@pytest.mark.parametrize("name", ["config", "jorge_rho"])
def test_cells_at_a_million_paths(name):
    cfgd = SCENARIOS[name]
    months = [300, 120, 240, 299]
    _check(cfgd, SEED, 1_000_000, 12_345, months, _rows(cfgd["monthly_expenses"], months, 16))


def test_rows_equal_expense_probes():
    cfgd = SCENARIOS["jorge_rho"]
    p = params_from_config(Config(**cfgd))
    months = [180, 60, 240, 61, 180]
    rows = _rows(cfgd["monthly_expenses"], months, 15)
    grid = E.probe_grid(p, SEED, 0, 0, 50_000, months, rows).cpu().numpy()
    for c, (wm, row) in enumerate(zip(months, rows)):
        assert grid[c].tolist() == E.probe_expenses(p, SEED, 0, 0, 50_000, wm, row).cpu().numpy().tolist()


def test_numpy_stream_agrees_with_per_cell_launches():
    cfgd = SCENARIOS["config"]
    months = [37, 0, 233, 37]
    rng = N.numpy_rng(1234, child_offset=0)
    _check(cfgd, rng, 1000, 0, months, _rows(cfgd["monthly_expenses"], months, 5), stream=1)


def test_limits():
    cfgd = SCENARIOS["config"]
    base = cfgd["monthly_expenses"]
    # one distinct month (once and repeated): the expense probe over the rows' levels
    for months in ([240], [240, 240, 240]):
        _check(cfgd, SEED, 2000, 0, months, _rows(base, months, 6))
    # one level per month
    months = [120, 240, 0, 301]
    _check(cfgd, SEED, 2000, 0, months, _rows(base, months, 1))
    # 32 distinct months (the most one accumulation sweep stores), then 40 rows of them: rows equal expense probes
    p = params_from_config(Config(**cfgd))
    months32 = [int(m) for m in np.random.default_rng(5).permutation(np.arange(0, 32 * 11, 11))]
    for months in (months32, months32 + months32[:8]):
        rows = _rows(base, months, 15)
        grid = E.probe_grid(p, SEED, 0, 0, 3000, months, rows).cpu().numpy()
        for c, (wm, row) in enumerate(zip(months, rows)):
            assert grid[c].tolist() == E.probe_expenses(p, SEED, 0, 0, 3000, wm, row).cpu().numpy().tolist(), (c, wm)
    assert E.probe_grid(p, SEED, 0, 0, 100, [], []).shape == (0, 0, 2)
    assert E.probe_grid(p, SEED, 0, 0, 100, [12, 24], [[], []]).shape == (2, 0, 2)


def test_invalid_input_leaves_counts_untouched():
    import torch

    p = params_from_config(Config(**SCENARIOS["config"]))
    lib = N.load_library()
    rng = N.McrRng()
    rng.kind, rng.philox_seed = N.MCR_RNG_PHILOX, SEED
    stream = torch.cuda.current_stream(0).cuda_stream
    sentinel = -0x1234_5678

    def call(months, levels, n_levels):
        counts = torch.full((max(1, len(months)), max(1, n_levels), 2), sentinel, dtype=torch.int64, device="cuda")
        m = (C.c_int32 * max(1, len(months)))(*months)
        lv = (C.c_double * max(1, len(levels)))(*levels)
        rc = lib.mcr_probe_grid_rng(C.byref(p), C.byref(rng), 0, 0, 1000, m, len(months), lv, n_levels,
                                    C.c_void_p(counts.data_ptr()), 0, C.c_void_p(stream))
        msg = N.last_error()
        torch.cuda.synchronize()
        return rc, msg, bool((counts.cpu() == sentinel).all())

    for bad in (float("nan"), -0.01, float("inf")):
        rc, msg, untouched = call([12, 24], [1000.0, 2000.0, 3000.0, bad], 2)
        assert rc == -1 and "monthly_expenses[1][1]" in msg and untouched
    for bad_month in (-1, 2**29):
        rc, msg, untouched = call([12, bad_month], [1000.0, 2000.0], 1)
        assert rc == -1 and untouched
    assert call([], [], 3)[0] == 0 and call([], [], 3)[2]
    assert call([12, 24], [], 0)[0] == 0 and call([12, 24], [], 0)[2]
    with pytest.raises(RuntimeError, match="monthly_expenses"):
        E.probe_grid(p, SEED, 0, 0, 100, [12, 24], [[1.0], [float("nan")]])
    with pytest.raises(ValueError):
        E.probe_grid(p, SEED, 0, 0, 100, [12, 24], [[1.0, 2.0], [3.0]])


@pytest.mark.parametrize("rng", ["philox", "numpy"])
def test_class_grid_rows_equal_probabilities_by_expenses(rng):
    cfgd = dict(SCENARIOS["jorge_rho"], seed=4242)
    sim = RetirementMonteCarloSimulator(Config(**cfgd), rng=rng)
    sim.use_search_seeds()
    months, levels = [150, 90, 150, 200], [3500.0, 0.0, 5200.5, 3500.0, 2100.0]
    got = sim.success_probability_grid(months, levels, 3000)
    assert got.dtype == np.float64 and got.shape == (len(months), len(levels))
    for c, wm in enumerate(months):
        assert got[c].tolist() == sim.success_probability_by_expenses(wm, levels, 3000).tolist(), wm


@pytest.mark.parametrize("name", ["config.json", "jorge.json"])
def test_frontier_equals_per_month_searches(name):
    cfgd = _cfg(name, seed=99)
    months = [120, 180, 240, 300]
    sim = RetirementMonteCarloSimulator(Config(**cfgd))
    events = []
    frontier = sim.find_maximum_monthly_expenses_by_months(months, verbose=False, progress_callback=events.append)
    assert len(frontier) == len(months)
    for wm, res in zip(months, frontier):
        single_events = []
        want = sim.find_maximum_monthly_expenses(wm, verbose=False, progress_callback=single_events.append)
        assert res == want, wm
        mine = [e for e in events if e["working_months"] == wm]
        assert [{k: v for k, v in e.items() if k != "working_months"} for e in mine] == single_events


def _cli(*args):
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--seed", "7", *args]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_cli_frontier_and_grid():
    out = _cli("--search-paths", "5000", "--frontier", "180,240,300")
    assert [o["working_months"] for o in out] == [180, 240, 300]
    for o in out:
        assert set(o) == {"working_months", "max_monthly_expenses", "probability", "levels_evaluated"}
        assert o["max_monthly_expenses"] > 0 and o["probability"] >= 97.0 and o["levels_evaluated"] > 0
    assert out[0]["max_monthly_expenses"] <= out[2]["max_monthly_expenses"]
    g = _cli("--paths", "4000", "--grid-months", "180,240", "--grid-expenses", "3000,4000,5000")
    assert g["working_months"] == [180, 240] and g["monthly_expenses"] == [3000.0, 4000.0, 5000.0]
    table = np.array(g["probability"])
    assert table.shape == (2, 3) and ((0 <= table) & (table <= 100)).all()
