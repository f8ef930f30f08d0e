"""Yearly bins taken INSIDE the path kernel (mcr_run_year_bins_rng): every table row against np.histogram of the kernel's
own full-output trajectories (bit-identical values: every cell equal), against the CPU oracle (a path within 1e-8 of an
edge may sit on either side), and the brackets of `bands_from_bins` against the exact radix-select route."""

from __future__ import annotations

import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import bin_rule
from conftest import REPO, load_golden
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import aggregation as A
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd import results as R
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

pytestmark = pytest.mark.gpu
TABLES = ("trajectory_bins", "real_trajectory_bins", "wr_bins", "final_success_bins")
BLOCKS = ("counters", "wr_obs_counts", "ruin_year_bins") + TABLES


def _cfg(name="config.json", **over):
    with open(os.path.join(REPO, "scenarios", name)) as fh:
        return Config(**dict(json.load(fh), seed=12345, **over))


def _jorge():
    return params_from_config(_cfg("jorge.json", equity_inflation_correlation=0.3))


def _cells(row, edges):
    row = row[~np.isnan(row)]
    return np.concatenate(([np.count_nonzero(row < edges[0])], np.histogram(row, bins=edges)[0],
                           [np.count_nonzero(row > edges[-1])])).astype(np.int64)


def _expected(full, edges, wr_edges):
    ok = full["success"].astype(bool)
    return {
        "trajectory_bins": np.stack([_cells(r, edges) for r in full["trajectory"]]),
        "real_trajectory_bins": np.stack([_cells(r, edges) for r in full["real_trajectory"]]),
        "wr_bins": np.stack([_cells(r, wr_edges) for r in full["withdrawal_rate_trajectory"]]),
        "final_success_bins": _cells(full["final_balance"][ok], edges),
    }


def _check_exact(p, seed, n, wm, edges, wr_edges, full=None, count_only=None, **kw):
    """The four tables of one launch equal np.histogram of the full-output launch's rows, cell for cell."""
    if full is None:
        full = E.run_batch_host(p, seed, 1, 0, n, wm, **kw)
    yb = E.run_year_bins_host(p, seed, 1, 0, n, wm, edges=edges, wr_edges=wr_edges, **kw)
    exp = _expected(full, yb["edges"], yb["wr_edges"])
    for k in TABLES:
        assert np.array_equal(yb[k].astype(np.int64), exp[k]), k
    assert np.all(yb["trajectory_bins"].sum(axis=1) == n) and np.all(yb["real_trajectory_bins"].sum(axis=1) == n)
    assert np.array_equal(yb["wr_bins"].sum(axis=1), yb["wr_obs_counts"])
    assert int(yb["final_success_bins"].sum()) == int(yb["counters"][0])
    if count_only is None:
        count_only = E.run_batch_host(p, seed, 1, 0, n, wm, want_summary=False, want_trajectories=False, **kw)
    for k in ("counters", "wr_obs_counts", "ruin_year_bins"):
        assert yb[k].tolist() == count_only[k].tolist() == full[k].tolist(), k
    return full, yb


@pytest.fixture(scope="module")
def jorge_full():
    """Full-output and count-only launches of 5 003 jorge.json paths (ragged last workgroup) per working-month count."""
    p = _jorge()
    out = {}
    for wm in (0, 75, 120):
        full = E.run_batch_host(p, 99, 1, 0, 5003, wm)
        cnt = E.run_batch_host(p, 99, 1, 0, 5003, wm, want_summary=False, want_trajectories=False)
        out[wm] = (full, cnt)
    return p, out


@pytest.mark.parametrize("wm", [0, 75, 120])
def test_tables_equal_histograms_of_the_kernels_own_trajectories(jorge_full, wm):
    """wm = 75: the terminal partial period rewrites row T - 1 of successful paths, and there is an extra row at retirement."""
    p, runs = jorge_full
    full, cnt = runs[wm]
    top = float(full["trajectory"].max())
    edge_sets = {
        "default64": E.default_year_edges(64),
        "one_bin": np.array([0.0, top]),
        "max_bins": E.default_year_edges(N.MCR_MAX_YEAR_BINS),
        "zero_width": np.array([0.0, 0.1, 0.1, 0.1, 0.5, 0.5, 0.8, 1.0]) * top,
        "edge_at_zero_inside": np.array([-1e6, 0.0, 1e5, 1e6, 1e7, 1e12]),
        "mostly_above": np.array([0.0, 10.0, 100.0, 1000.0]),
    }
    wr_sets = {"default64": E.default_wr_edges(64), "one_bin": np.array([0.0, 1000.0]), "max_bins": E.default_wr_edges(N.MCR_MAX_YEAR_BINS, 50.0),
               "zero_width": np.array([0.0, 4.0, 4.0, 8.0, 8.0, 100.0]), "mostly_above": np.array([0.0, 0.5, 1.0])}
    for name, edges in edge_sets.items():
        _, yb = _check_exact(p, 99, 5003, wm, edges, wr_sets.get(name, wr_sets["default64"]), full=full, count_only=cnt)
        if name == "mostly_above" and wm > 0:      # (retiring at once, most samples are the exact zeros of failed paths)
            assert yb["trajectory_bins"][1:, -1].sum() > 0.5 * yb["trajectory_bins"][1:].sum()
    if wm == 75:
        sz = E.query_sizes(p, wm)
        assert sz.total_months % 12 != 0 and sz.trajectory_len == 1 + 6 + 1 + sz.retirement_years


def test_mostly_failing_plan_reaches_the_pad_loop():
    cfg = _cfg(monthly_expenses=14_000.0)
    p = params_from_config(cfg)
    n, wm = 2048, 233
    full = E.run_batch_host(p, 7, 1, 0, n, wm)
    assert full["success"].mean() < 0.4
    ry = full["withdrawal_rate_trajectory"].shape[0]
    dead_before_last = np.isnan(full["withdrawal_rate_trajectory"][ry - 2]).reshape(-1, 64).all(axis=1)
    assert dead_before_last.any(), "no 64-path wave has every lane failed before the last year"
    _check_exact(p, 7, n, wm, E.default_year_edges(64), E.default_wr_edges(64), full=full)


def test_annual_gains_tax_scenarios_and_pre_retirement_failures():
    """Every tax configuration of helpers.json (retirement_years = 30, wm = 61, n = 2 048; [5] is the issue's, [1] and [2]
    carry an annual-gains tax: the ANNUAL kernel variants).  None of the six has a pre-retirement tax failure at this shape
    (asserted below), so that trap is reached through the golden scenario built for it, paths_deterministic.json
    'pre_retirement_tax_failure' (every path fails in the accumulation), and a variant of it with volatile returns: waves that
    hold failed and live lanes together."""
    cfgs = load_golden("helpers.json")["tax_cfgs"]
    assert len(cfgs) == 6
    for c in cfgs:
        p = params_from_config(Config(**dict(c, retirement_years=30, seed=7)))
        full, _ = _check_exact(p, 12345, 2048, 61, E.default_year_edges(64), E.default_wr_edges(64))
        assert int(full["ruin_year_bins"][0]) == 0          # (else this configuration would do, as the issue says)
    g = [x for x in load_golden("paths_deterministic.json") if x["name"] == "pre_retirement_tax_failure"][0]
    for over in ({}, {"inv1_returns_volatility": 0.6, "inv2_premium_over_inflation_volatility": 0.3}):
        p = params_from_config(Config(**dict(g["cfg"], **over)))
        full, yb = _check_exact(p, 12345, 2048, g["working_months"], E.default_year_edges(64), E.default_wr_edges(64))
        if not over:
            assert int(full["ruin_year_bins"][0]) == 2048           # every path: YearsToRuin 0.0, zeros from retirement on
            assert int(yb["wr_bins"].sum()) == 0
        else:
            assert 0 < int(full["ruin_year_bins"][0]) < 2048        # a mix
            pre = np.isnan(full["withdrawal_rate_trajectory"][0]) & (full["years_to_ruin"] == 0.0)
            mixed = pre.reshape(-1, 64).any(axis=1) & ~pre.reshape(-1, 64).all(axis=1)
            assert mixed.any(), "no 64-path wave holds pre-retirement failures and live lanes together"


def test_numpy_stream_and_long_stream_lists():
    p = _jorge()
    full = E.run_batch_host(p, N.numpy_rng(2024), 1, 0, 1500, 75)
    cnt = E.run_batch_host(p, N.numpy_rng(2024), 1, 0, 1500, 75, want_summary=False, want_trajectories=False)
    yb = E.run_year_bins_host(p, N.numpy_rng(2024), 1, 0, 1500, 75, edges=E.default_year_edges(64), wr_edges=E.default_wr_edges(64))
    exp = _expected(full, yb["edges"], yb["wr_edges"])
    for k in TABLES:
        assert np.array_equal(yb[k].astype(np.int64), exp[k]), k
    assert yb["counters"].tolist() == cnt["counters"].tolist()
    # 20 income streams: the generic variant (device table of the records beyond the by-value block)
    d = dict(load_golden("helpers.json")["tax_cfgs"][5])
    streams = [{"name": f"s{i}", "monthly_amount_today": 60.0 + 15 * (i % 11), "start_at_age": 37.0 + 0.9 * i,
                "duration_years": [None, 0, 1, 3, 7, 12][i % 6], "inflation_indexed": i % 2 == 0, "tax_rate": 0.05 * (i % 5)}
               for i in range(20)]
    d.update(initial_balance=800_000.0, monthly_contribution=1_000.0, monthly_expenses=4_300.0, retirement_years=28,
             inv1_returns_volatility=0.17, other_income_streams=streams, seed=7)
    pm = params_from_config(Config(**d))
    assert pm.n_streams == 20 and bool(pm.extra_streams)
    _check_exact(pm, 77, 1024, 61, E.default_year_edges(64), E.default_wr_edges(64))


def test_accumulation_device_list_and_batch_views(jorge_full):
    import torch

    p, runs = jorge_full
    n, wm = 5003, 75
    e, we = E.default_year_edges(64), E.default_wr_edges(64)
    one = E.run_year_bins_host(p, 99, 1, 0, n, wm, edges=e, wr_edges=we)
    half = E.run_year_bins_host(p, 99, 1, 0, n // 2, wm, edges=e, wr_edges=we)
    E.run_year_bins_host(p, 99, 1, n // 2, n - n // 2, wm, edges=e, wr_edges=we, into=half)
    three = E.run_year_bins_host(p, 99, 1, 0, n, wm, edges=e, wr_edges=we, devices=[0, 0, 0])
    for k in BLOCKS:
        assert np.array_equal(one[k], half[k]), k
        assert np.array_equal(one[k], three[k]), k
    # a device list on top of nonzero caller tables: the shards' sums are added to what is there
    onto = E.run_year_bins_host(p, 99, 1, 0, n // 2, wm, edges=e, wr_edges=we)
    E.run_year_bins_host(p, 99, 1, n // 2, n - n // 2, wm, edges=e, wr_edges=we, into=onto, devices=[0, 0, 0])
    # fewer paths than shards: ceil(2 / 3) = 1 path each, the last shard is empty
    two = E.run_year_bins_host(p, 99, 1, 0, 2, wm, edges=e, wr_edges=we)
    sparse = E.run_year_bins_host(p, 99, 1, 0, 2, wm, edges=e, wr_edges=we, devices=[0, 0, 0])
    for k in BLOCKS:
        assert np.array_equal(one[k], onto[k]), k
        assert np.array_equal(two[k], sparse[k]), k
    b = E.YearBinsBatch(p, wm, e, we)
    b.launch(99, 1, 0, n // 2)
    b.launch(99, 1, n // 2, n - n // 2)
    host = b.host()
    for k in BLOCKS:
        assert np.array_equal(host[k].astype(np.uint64), one[k]), k
    at = b.reduce_vec.data_ptr()
    for k in BLOCKS:                                   # the named views alias the one vector, in order, with no gaps
        v = getattr(b, k)
        assert v.data_ptr() == at and v.is_contiguous()
        at += v.numel() * 8
    assert at == b.reduce_vec.data_ptr() + b.reduce_vec.numel() * 8
    b.wr_obs_counts.zero_()
    assert int(b.reduce_vec[2:2 + b.sizes.retirement_years].sum()) == 0
    del b
    torch.cuda.empty_cache()


def test_argument_errors_leave_the_tables_untouched():
    lib = N.load_library()
    p = _jorge()
    sz = E.query_sizes(p, 75)
    T, ry = sz.trajectory_len, sz.retirement_years
    good = E.default_year_edges(64)

    def call(edges=good, n_bins=64, wr_edges=E.default_wr_edges(16), n_wr=16, null_edges=False, per_path=False):
        e = np.ascontiguousarray(edges, dtype=np.float64)
        we = np.ascontiguousarray(wr_edges, dtype=np.float64)
        cells = max(n_bins, 1) + 2
        tabs = [np.full((T, cells), 7, dtype=np.uint64), np.full((T, cells), 7, dtype=np.uint64),
                np.full((ry, max(n_wr, 1) + 2), 7, dtype=np.uint64), np.full(cells, 7, dtype=np.uint64)]
        ctr = np.full(2, 7, dtype=np.uint64)
        o = N.McrOutputs()
        o.counters = ctr.ctypes.data
        extra = np.zeros(8)
        if per_path:
            o.final_balance = extra.ctypes.data
        y = N.McrYearBins()
        y.edges, y.n_bins, y.wr_edges, y.n_wr_bins = (None if null_edges else e.ctypes.data), n_bins, we.ctypes.data, n_wr
        y.trajectory_bins, y.real_trajectory_bins, y.wr_bins, y.final_success_bins = (t.ctypes.data for t in tabs)
        rng = N.philox_rng(5)
        rc = lib.mcr_run_year_bins_host_rng(C.byref(p), C.byref(rng), 1, 0, 8, 75, C.byref(o), C.byref(y), 0)
        untouched = all(np.all(t == 7) for t in tabs) and np.all(ctr == 7)
        return rc, untouched

    assert call() [0] == 0
    bad = dict(
        descending=dict(edges=good[::-1]), nan=dict(edges=np.where(np.arange(65) == 9, np.nan, good)),
        wr_descending=dict(wr_edges=E.default_wr_edges(16)[::-1]), null_edges=dict(null_edges=True),
        zero_bins=dict(n_bins=0), negative_bins=dict(n_bins=-1), too_many=dict(n_bins=N.MCR_MAX_YEAR_BINS + 1, edges=np.arange(N.MCR_MAX_YEAR_BINS + 2.0)),
        wr_zero=dict(n_wr=0), per_path_pointer=dict(per_path=True),
    )
    for name, kw in bad.items():
        rc, untouched = call(**kw)
        assert rc == N.MCR_ERR_INVALID_ARG == -1, (name, rc)
        assert untouched, name
    # injected shocks: the entry points have no argument for them, and the Python face takes none either
    with pytest.raises(TypeError):
        E.run_year_bins_host(p, 5, 1, 0, 8, 75, injected_shocks=np.zeros((8, sz.shock_rows, 3)))


@pytest.mark.parametrize("scenario", ["s60", "jorge"])
def test_tables_vs_oracle(oracle, scenario):
    """20 000 paths against np.histogram of the ORACLE's rows (reference arithmetic): a row that is not exactly equal may move
    at most 2 x (its entries within 1e-8 relative of an edge), the rule of test_bins_vs_oracle_1e5 per row, as tests/bin_rule.py
    states it: the edge at 0 of the default edges moves nothing, and no entry lies below it."""
    if scenario == "s60":
        p, wm = params_from_config(_cfg(initial_balance=2.0e6, inv1_returns_volatility=0.15, equity_inflation_correlation=0.3)), 120
    else:
        p, wm = _jorge(), 75
    n = 20_000
    c = oracle.run_batch(p, 12345, 1, 1 << 33, n, wm, want_trajectories=True)
    yb = E.run_year_bins_host(p, 12345, 1, 1 << 33, n, wm, edges=E.default_year_edges(64), wr_edges=E.default_wr_edges(64))
    assert yb["counters"].tolist() == c["counters"].tolist()
    ok = c["success"].astype(bool)
    rows = [("trajectory_bins", c["trajectory"], yb["edges"]), ("real_trajectory_bins", c["real_trajectory"], yb["edges"]),
            ("wr_bins", c["withdrawal_rate_trajectory"], yb["wr_edges"]), ("final_success_bins", c["final_balance"][ok][None, :], yb["edges"])]
    for name, data, edges in rows:
        got = yb[name].astype(np.int64).reshape(data.shape[0], -1)
        for t, row in enumerate(data):
            bin_rule.check_row(got[t], row, edges, f"{name}[{t}]")


def test_brackets_contain_the_exact_bands_and_the_streamed_document():
    import torch

    cfg = _cfg("jorge.json", equity_inflation_correlation=0.3)
    p = params_from_config(cfg)
    n, wm = 20_000, 75
    batch = E.DeviceBatch(p, wm, n, want="full")
    batch.launch(12345, 1, 0)
    traj_q, real_q, wr_q, _ = A.band_quantiles(batch, n)
    del batch
    torch.cuda.empty_cache()
    yb = E.run_year_bins_host(p, 12345, 1, 0, n, wm)           # the default edges
    for name, exact, edges, qs in (("trajectory_bins", traj_q, yb["edges"], A.TRAJECTORY_QUANTILES),
                                   ("real_trajectory_bins", real_q, yb["edges"], A.TRAJECTORY_QUANTILES),
                                   ("wr_bins", wr_q, yb["wr_edges"], A.WR_QUANTILES)):
        lo, hi, est = A.bands_from_bins(yb[name], edges, qs)
        both = np.isfinite(lo) & np.isfinite(hi) & ~np.isnan(exact)
        assert np.all(lo[both] <= exact[both]) and np.all(exact[both] <= hi[both]), name
        if name != "wr_bins":
            assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)), f"{name}: a quantile outside the default edges"
    # the same through the documents
    sim = RetirementMonteCarloSimulator(cfg, main_seed_override=2024)
    sim.use_final_seeds()
    compact = json.loads(json.dumps(R.compact_result(cfg, sim, wm, num_simulations=n)))
    sim2 = RetirementMonteCarloSimulator(cfg, main_seed_override=2024)
    sim2.use_final_seeds()
    doc = json.loads(json.dumps(R.streamed_result(cfg, sim2, wm, num_simulations=n)))
    assert set(compact) <= set(doc)
    assert doc["not_available"] == ["summary.swr"] and doc["summary"]["swr"] is None
    for k in ("success_probability", "required_working_months", "retirement_age", "target_probability"):
        assert doc["summary"][k] == compact["summary"][k], k
    assert doc["ruin_histogram"] == compact["ruin_histogram"]
    assert doc["withdrawal_rate"]["observation_counts"] == compact["withdrawal_rate"]["observation_counts"]
    assert doc["reference_lines"] == compact["reference_lines"]
    for fam in ("trajectory", "trajectory_real"):
        assert doc[fam]["sample_paths"] == compact[fam]["sample_paths"] and len(doc[fam]["sample_paths"]) == 5
        assert doc[fam]["years"] == compact[fam]["years"]

    def inside(lo, x, hi, what):
        for a, v, b in zip(lo, x, hi):
            if a is not None and b is not None and v is not None:
                assert a - 0.01 <= v <= b + 0.01, (what, a, v, b)

    for fam in ("trajectory", "trajectory_real", "withdrawal_rate"):
        br = doc["band_brackets"][fam]
        for key, exact in compact[fam]["percentiles"].items():
            inside(br["lo"][key], exact, br["hi"][key], (fam, key))
            inside(br["lo"][key], doc[fam]["percentiles"][key], br["hi"][key], (fam, key, "estimate"))
    br = doc["band_brackets"]
    inside(br["median_start_balance"]["lo"]["p50"], [compact["summary"]["median_start_balance"]], br["median_start_balance"]["hi"]["p50"], "start")
    inside(br["median_final_balance_successful"]["lo"]["p50"], [compact["summary"]["median_final_balance_successful"]],
           br["median_final_balance_successful"]["hi"]["p50"], "final ok")
    for key, exact in compact["summary"]["final_balance_percentiles"].items():
        inside(br["final_balance_percentiles"]["lo"][key], [exact], br["final_balance_percentiles"]["hi"][key], ("final", key))
    # edges that miss the data: the medians are None and named, never a made-up 0.0
    sim3 = RetirementMonteCarloSimulator(cfg, main_seed_override=2024)
    sim3.use_final_seeds()
    off = json.loads(json.dumps(R.streamed_result(cfg, sim3, wm, num_simulations=2000, edges=[1e13, 1e14, 1e15])))
    assert off["summary"]["median_start_balance"] is None and off["summary"]["median_final_balance_successful"] is None
    assert set(off["not_available"]) == {"summary.swr", "summary.median_start_balance", "summary.median_final_balance_successful"}
    assert all(v is None for v in off["trajectory"]["percentiles"]["p50"])
    assert off["summary"]["success_probability"] > 0
    hb = doc["histogram_binned"]
    assert sum(hb["success_counts"]) + hb["below"] + hb["above"] == hb["successful_paths"] == compact["histogram_binned"]["successful_paths"]


def test_two_ranks_one_all_reduce(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res")
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "dist_year_bins_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for pr in procs:
        stdout, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, stdout.decode()[-3000:]
    whole = E.run_year_bins_host(_jorge(), 2024, 1, 0, 10_007, 75, edges=E.default_year_edges(64), wr_edges=E.default_wr_edges(64))
    vec = np.concatenate([whole[k].reshape(-1) for k in BLOCKS]).astype(np.int64)
    for rank in range(2):
        r = json.load(open(f"{out}.{rank}"))
        assert r["vector"] == vec.tolist(), rank
        assert r["exchange"] == f"1 all-reduce(sum) of {vec.size} int64 words"
        assert r["collectives"] == 1


def test_cli_streamed(tmp_path):
    cfg = json.load(open(os.path.join(REPO, "scenarios", "jorge.json")))
    cfg.update(num_simulations_main=3000, seed=11)
    path = tmp_path / "scenario.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "run_scenario.py"), str(path), "--working-months", "75",
                          "--streamed", "--full"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    start = out.stdout.index("{")
    doc = json.loads(out.stdout[start:])
    doc = doc.get("result", doc)
    assert doc["not_available"] == ["summary.swr"] and "band_brackets" in doc
    assert len(doc["trajectory"]["percentiles"]["p50"]) == len(doc["trajectory"]["years"])
    assert doc["histogram_binned"]["total_paths"] == 3000
