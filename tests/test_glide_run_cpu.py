"""The glide whole-path launches (`mcr_run_glide_rng`, `mcr_run_glide_year_bins_rng`, `mcr_run_glide_year_bins_host_rng`) without
a GPU: the three entry points in header, binding and library (ABI still v8); the host-side validation, which names its field
before a device is looked for and leaves every output alone; what the Python surface refuses; and the allowance that the bin
rule of tests/bin_rule.py can grant the GPU comparison of tests/test_gpu_glide_run_vs_oracle.py, pinned.

THE ALLOWANCE.  The yearly tables of a glide launch are compared with the model (tests/glide_model.cpp) through `bin_rule`: a row
that is not equal cell for cell may move by twice its entries within 1e-8 (relative) of an edge.  Here the model runs every plan
of the six served classes of tests/count_fuzz.py under the five tables of tests/glide_fuzz.py, and the yearly samples (nominal
balance, real balance, withdrawal rate) that lie so near an edge of `engine.default_year_edges()` / `default_wr_edges()` are
counted: at most 2 over all classes (measured with the suite's seed: 2, both in class `mask0`), so the GPU comparison can hide at
most four moved cells of the yearly tables in the whole suite.  (`final_success_bins` holds the last trajectory sample of the paths
that succeed: its entries near an edge are among those counted.)  And the plans are mixed: at least 40 of the 50 runs of each
class have a failure share strictly between 0 and 1 (measured: 41 to 48)."""

from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bin_rule
import count_fuzz as F
import glide_fuzz as GF
import spending_rule_model as M
from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd import results as R
from monte_carlo_retirement_amd.spending_rules import SpendingRule

SYMBOLS = ("mcr_run_glide_rng", "mcr_run_glide_year_bins_rng", "mcr_run_glide_year_bins_host_rng")
SERVED = tuple(c for c in F.CLASSES if c != "generic")
WM = 7
ENTRIES = ("count", "bins", "bins_host")


@pytest.fixture(scope="module")
def lib():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    return N.load_library()


def test_header_binding_and_library_agree(lib):
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert int(re.search(r"#define MCR_ABI_VERSION (\d+)", header).group(1)) == N.MCR_ABI_VERSION == 8
    assert lib.mcr_abi_version() == 8
    declared = set(re.findall(r"\b(mcr_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in SYMBOLS:
        assert name in declared and name in N.ABI_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes[6:8] == [C.POINTER(C.c_double), C.c_int32], name      # weights, n_weights
    assert "There is NO plain launch" not in header and "Glide whole-path launches" in header


def _params(**over):
    cfg = dict(M.plan_config("realized", REPO, WM), monthly_expenses=M.LEVELS["realized", WM]["symmetric"])
    cfg.update(over)
    return params_from_config(Config(**cfg))


class Call:
    """One call of an entry point with sentinel-filled outputs (HOST arrays: a refusal comes before a device is looked for, so the
    device forms never read them); `run` returns (rc, message, whether every output is untouched)."""

    def __init__(self, lib):
        self.lib = lib

    def run(self, entry, weights=(0.6, 0.5), n_weights=None, null_weights=False, rng=None, edges=None, wr_edges=None, trajectory=False,
            hist=False, params=None, n_bins=16, n_wr=8):
        p = _params() if params is None else params
        sz = E.query_sizes(p, WM)
        T, ry = sz.trajectory_len, sz.retirement_years
        e = np.ascontiguousarray(E.default_year_edges(n_bins) if edges is None else edges, dtype=np.float64)
        we = np.ascontiguousarray(E.default_wr_edges(n_wr) if wr_edges is None else wr_edges, dtype=np.float64)
        outs = [np.full(2, 7, dtype=np.uint64), np.full(ry, 7, dtype=np.uint64), np.full(sz.ruin_bins, 7, dtype=np.uint64),
                np.full((T, n_bins + 2), 7, dtype=np.uint64), np.full((T, n_bins + 2), 7, dtype=np.uint64), np.full((ry, n_wr + 2), 7, dtype=np.uint64),
                np.full(n_bins + 2, 7, dtype=np.uint64), np.full((T, 8), -7.0), np.full(4, 7, dtype=np.uint64)]
        o = N.McrOutputs()
        o.counters, o.wr_obs_counts, o.ruin_year_bins = (t.ctypes.data for t in outs[:3])
        o.path_stride = 8
        hist_edges = np.linspace(0.0, 1e6, 5)
        if trajectory:
            o.trajectory = outs[7].ctypes.data
        if hist:
            o.hist_bins, o.hist_edges, o.hist_n_bins = outs[8].ctypes.data, hist_edges.ctypes.data, 4
        y = N.McrYearBins()
        y.edges, y.n_bins, y.wr_edges, y.n_wr_bins = e.ctypes.data, n_bins, we.ctypes.data, n_wr
        y.trajectory_bins, y.real_trajectory_bins, y.wr_bins, y.final_success_bins = (t.ctypes.data for t in outs[3:7])
        w = (C.c_double * max(1, len(weights)))(*weights)
        nw = len(weights) if n_weights is None else n_weights
        g = N.philox_rng(5) if rng is None else rng
        head = (C.byref(p), C.byref(g), 1, 0, 8, WM, None if null_weights else w, nw, C.byref(o))
        if entry == "count":
            rc = self.lib.mcr_run_glide_rng(*head, 0, None)
        elif entry == "bins":
            rc = self.lib.mcr_run_glide_year_bins_rng(*head, C.byref(y), 0, None)
        else:
            rc = self.lib.mcr_run_glide_year_bins_host_rng(*head, C.byref(y), 0)
        untouched = all(np.all(t == 7) for t in outs[:7]) and np.all(outs[7] == -7.0) and np.all(outs[8] == 7)
        return rc, N.last_error(), untouched


def test_validation_names_the_field_before_any_device_work(lib):
    """Every refusal below comes from the host-side checks: the same code and message with or without a GPU in the box, and every
    output keeps its sentinel."""
    call = Call(lib)
    history = N.history_rng(3, np.random.default_rng(1).standard_normal((240, 3)), 12)
    many = dict(M.plan_config("realized", REPO, WM))
    many["other_income_streams"] = [{"name": f"s{k}", "monthly_amount_today": 100.0 + k, "start_at_age": 50.0 + k, "duration_years": None,
                                     "inflation_indexed": True, "tax_rate": 0.1} for k in range(17)]
    p17 = params_from_config(Config(**many))
    exact = _params(inv1_use_realized_gains_tax_system=True, inv1_realized_gains_tax_rate=1.0 - 1e-7)
    cases = [
        ("null weights", dict(null_weights=True), N.MCR_ERR_INVALID_ARG, "weights"),
        ("n_weights 0", dict(n_weights=0), N.MCR_ERR_INVALID_ARG, "n_weights"),
        ("a NaN weight", dict(weights=(0.5, float("nan"))), N.MCR_ERR_INVALID_ARG, "weights[1]"),
        ("a weight of -0.01", dict(weights=(-0.01,)), N.MCR_ERR_INVALID_ARG, "weights[0]"),
        ("a weight of 1.01", dict(weights=(0.2, 0.3, 1.01)), N.MCR_ERR_INVALID_ARG, "weights[2]"),
        ("the NumPy stream", dict(rng=N.numpy_rng(12345)), N.MCR_ERR_UNSUPPORTED, "glide path: the NumPy stream is not supported"),
        ("the history stream", dict(rng=history), N.MCR_ERR_UNSUPPORTED, "glide path: the history stream is not supported"),
        ("a trajectory pointer", dict(trajectory=True), N.MCR_ERR_UNSUPPORTED, "glide path: trajectories are not supported"),
        ("17 streams", dict(params=p17), N.MCR_ERR_UNSUPPORTED, "glide path: 17 income streams"),
        ("the exact month", dict(params=exact), N.MCR_ERR_UNSUPPORTED, "glide path: the exact month"),
    ]
    for name, kw, code, word in cases:
        for entry in ENTRIES:
            rc, msg, untouched = call.run(entry, **kw)
            assert rc == code and word in msg and untouched, (name, entry, rc, msg, untouched)
    rc, msg, untouched = call.run("count", hist=True)
    assert rc == N.MCR_ERR_UNSUPPORTED and "glide path: the in-kernel histogram (hist_bins) is not supported" in msg and untouched
    # the host form checks its edges
    good, good_wr = E.default_year_edges(16), E.default_wr_edges(8)
    for name, kw, word in [("unsorted edges", dict(edges=good[::-1]), "edges["),
                           ("a NaN edge", dict(edges=np.where(np.arange(17) == 5, np.nan, good)), "edges[5]"),
                           ("an infinite wr edge", dict(wr_edges=np.where(np.arange(9) == 8, np.inf, good_wr)), "wr_edges[8]"),
                           ("unsorted wr edges", dict(wr_edges=good_wr[::-1]), "wr_edges[")]:
        rc, msg, untouched = call.run("bins_host", **kw)
        assert rc == N.MCR_ERR_INVALID_ARG and word in msg and untouched, (name, rc, msg, untouched)


def _frozen(k):
    """A plan with k paying income streams that are not inflation-indexed: k lock columns in LDS."""
    return _params(other_income_streams=[{"name": f"f{i}", "monthly_amount_today": 200.0 + i, "start_at_age": 60.0 + i, "duration_years": None,
                                          "inflation_indexed": False, "tax_rate": 0.1} for i in range(k)])


def test_lock_columns_that_do_not_fit_beside_the_yearly_tables_are_refused(lib):
    """The yearly tables take LDS that a count-only launch leaves to the lock columns of frozen income streams, and the glide
    kernels have no generic form to put the rest in device memory.  A yearly-bins glide launch gives up resident workgroups for
    them (columns up to the workgroup's 64 KB: tests/test_gpu_glide_run.py runs such plans against the plain launch's generic
    form); what does not fit even then -- about 45 KB of tables at 512 + 512 bins leave 9 columns, 34 KB at 256 + 256 leave 14 --
    both yearly-bins entries refuse by name, before a device is looked for, and touch nothing.  (More than the eight columns a
    count-only launch has room for are refused first, by the rule the count-only and summary launches share; the yearly-bins
    plan's own refusal stands behind it for whatever that rule lets through.)"""
    call = Call(lib)
    for what, params, bins in (("ten frozen streams at 512 + 512 bins", _frozen(10), N.MCR_MAX_YEAR_BINS), ("sixteen frozen streams at the default edges", _frozen(16), 256)):
        for entry in ("bins", "bins_host"):
            rc, msg, untouched = call.run(entry, params=params, n_bins=bins, n_wr=bins)
            assert rc == N.MCR_ERR_UNSUPPORTED and "glide path:" in msg and "frozen income streams" in msg and untouched, (what, entry, rc, msg, untouched)


def test_launch_without_a_device_fails_loudly(lib):
    """There is no CPU fallback: valid arguments without a HIP device give MCR_ERR_NO_DEVICE from all three entry points.  (In a
    child process: a call that initialises the HIP runtime would hold the GPU open for the rest of the session.)  With a device,
    the same calls with no paths succeed."""
    code = ("import ctypes as C, json\n"
            "from monte_carlo_retirement_amd import Config, params_from_config\n"
            "from monte_carlo_retirement_amd import _native as N\n"
            "lib = N.load_library()\n"
            "p = params_from_config(Config(**json.load(open('tests/golden/paths_injected.json'))[0]['cfg']))\n"
            "rng, o, y, w = N.philox_rng(1), N.McrOutputs(), N.McrYearBins(), (C.c_double * 2)(0.6, 0.4)\n"
            "head = (C.byref(p), C.byref(rng), 1, 0, 0, 12, w, 2, C.byref(o))\n"
            "rcs = [lib.mcr_run_glide_rng(*head, 0, None)]\n"
            "msgs = [N.last_error().replace(' ', '_') or '-']\n"
            "rcs.append(lib.mcr_run_glide_year_bins_rng(*head, C.byref(y), 0, None))\n"
            "msgs.append(N.last_error().replace(' ', '_') or '-')\n"
            "rcs.append(lib.mcr_run_glide_year_bins_host_rng(*head, C.byref(y), 0))\n"
            "msgs.append(N.last_error().replace(' ', '_') or '-')\n"
            "print(lib.mcr_device_count(), *rcs, *msgs)")
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    devices, a, b, c, ma, mb, mc = r.stdout.split()[-7:]
    for rc, msg in ((a, ma), (b, mb), (c, mc)):
        if int(devices) > 0:
            assert int(rc) == 0, msg
        else:
            assert int(rc) == N.MCR_ERR_NO_DEVICE and "no_usable_HIP_device" in msg, (rc, msg)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def test_a_rule_together_with_a_glide_path_is_refused():
    p = _params()
    rule = SpendingRule(*M.RULES["symmetric"])
    with pytest.raises(ValueError, match="spending rule together with a glide path"):
        E.YearBinsBatch(p, WM, rule=rule, glide_path=[0.6, 0.5])
    with pytest.raises(ValueError, match="spending rule together with a glide path"):
        R.streamed_result(Config(**M.plan_config("realized", REPO, WM)), None, WM, rule=rule, glide_path=[0.6, 0.5])
    with pytest.raises(ValueError, match="at least one weight"):
        E.glide_table([])
    assert list(E.glide_table([0.25, 1])) == [0.25, 1.0]
    with pytest.raises(ValueError):
        E.run_glide_host(p, 1, 0, 0, 8, WM, [0.5], want="trajectories")


def test_allocation_by_sample_is_the_table():
    from monte_carlo_retirement_amd.allocation import GlidePath
    from monte_carlo_retirement_amd.simulation import allocation_by_sample, trajectory_sample_months, trajectory_time_points

    g = GlidePath([0.9, 0.8, 0.7, 0.6])
    for wm, ry in ((0, 3), (7, 2), (12, 2), (30, 4)):
        months = trajectory_sample_months(wm, ry)
        assert [m / 12 for m in months] == pytest.approx(trajectory_time_points(wm, ry), rel=1e-15, abs=0) and len(months) == len(trajectory_time_points(wm, ry))
        assert allocation_by_sample(g, wm, ry) == [g.weight_at(max(0, m - 1)) for m in months]
    assert allocation_by_sample(g, 30, 4) == [0.9, 0.9, 0.8, 0.7, 0.6, 0.6, 0.6, 0.6]     # months 0, 12, 24, 30, 42, 54, 66, 78
    assert allocation_by_sample(GlidePath.constant(0.3), 7, 2) == [0.3] * 4


def _cli(tmp_path, *flags):
    path = tmp_path / "scenario.json"
    if not path.exists():
        import json

        path.write_text(json.dumps(dict(M.plan_config("realized", REPO, WM), num_simulations_main=100)))
    return subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"), str(path), *flags],
                          capture_output=True, text=True, timeout=300)


def test_cli_refuses_malformed_and_conflicting_flags(tmp_path):
    rule = ",".join(str(x) for x in M.RULES["symmetric"])
    history = tmp_path / "history.csv"
    history.write_text("month,inv1,inflation,inv2\n")
    for flags, words in ((("--glide-path", "0.9>0.4@0-20", "--streamed"), "--glide-path needs --working-months"),
                         (("--working-months", "7", "--glide-path", "0.9>0.4@0-20", "--streamed", "--spending-rule", rule), "--glide-path and --spending-rule"),
                         (("--working-months", "7", "--glide-path", "0.9>0.4@0-20", "--streamed", "--history", str(history)), "engine's own stream"),
                         (("--working-months", "7", "--glide-path", "0.9>0.4@0-20", "--streamed", "--rng", "numpy"), "engine's own stream"),
                         (("--working-months", "7", "--glide-path", "0.9>0.4@0-20", "--streamed", "--glide-paths", "0.5;0.6"), "separate questions"),
                         (("--working-months", "7", "--glide-path", "0.9>0.4", "--streamed"), "--glide-path: glide path '0.9>0.4'"),
                         (("--working-months", "7", "--glide-path", "1.5", "--streamed"), "--glide-path:"),
                         (("--working-months", "7", "--glide-path", "0.5"), "--glide-path goes with --streamed"),
                         (("--working-months", "7", "--glide-path", "0.5", "--streamed", "--max-expenses"), "the other questions are separate")):
        out = _cli(tmp_path, *flags)
        assert out.returncode == 2 and words in out.stderr, (flags, out.returncode, out.stderr[-500:])


# ---- the allowance of the bin rule, pinned ----------------------------------------------------------------------------------------
def _near_an_edge(values, edges) -> int:
    """`bin_rule.near_an_edge` of `values`, asked only about the values within 1e-6 (relative) of a neighbouring edge: an entry
    within 1e-8 max(1, |e'|) of any edge e' is at least as close to the edge next to it, so none is left out."""
    values = values[~np.isnan(values)]
    k = np.searchsorted(edges, values)
    lo, hi = edges[np.clip(k - 1, 0, edges.size - 1)], edges[np.clip(k, 0, edges.size - 1)]
    close = (np.abs(values - lo) <= 1e-6 * np.maximum(1.0, np.abs(lo))) | (np.abs(values - hi) <= 1e-6 * np.maximum(1.0, np.abs(hi)))
    return bin_rule.near_an_edge(values[close], edges)


def test_the_allowance_of_the_bin_rule_is_at_most_two_entries(oracle):
    edges, wr_edges = E.default_year_edges(), E.default_wr_edges()
    near, samples = {}, 0
    for cls in SERVED:
        near[cls], mixed, runs_seen = 0, 0, 0
        for scn, runs in GF.class_runs(oracle, cls):
            for name, run in zip(GF.NAMES, runs):
                assert F.money_scale(run) < F.SCALE_LIMIT, (name, scn.context("glide run: money scale"))
                runs_seen += 1
                mixed += 0 < int(np.count_nonzero(run["success"])) < scn.n         # a failure share strictly between 0 and 1
                for key, e in (("trajectory", edges), ("real_trajectory", edges), ("withdrawal_rate_trajectory", wr_edges)):
                    v = run[key].reshape(-1)
                    samples += int(np.count_nonzero(~np.isnan(v)))
                    near[cls] += _near_an_edge(v, e)
        assert runs_seen == 50 and mixed >= 40, (cls, runs_seen, mixed)
        print(f"glide runs {cls}: {mixed} of {runs_seen} runs mixed, {near[cls]} yearly samples near an edge")
    print(f"{samples} yearly samples, near an edge per class: {near}")
    assert sum(near.values()) <= 2, near


def test_the_prefilter_counts_what_the_rule_counts():
    rng = np.random.default_rng(5)
    edges = E.default_year_edges(32)
    v = np.concatenate([rng.uniform(0, 1e6, 4000), edges[3:9] * (1 + 5e-9), edges[10:12] * (1 - 2e-8), [0.0, 0.0, np.nan, 1.0 + 1e-9]])
    assert _near_an_edge(v, edges) == bin_rule.near_an_edge(v, edges) >= 7


def test_the_integers_formed_from_the_columns_are_the_oracles(oracle):
    """tests/glide_run.py: `integers` of the oracle's own per-path columns equal the integers its batch loop keeps, for every
    plan of every served class (terminal-settlement failures and failures before retirement occur among them)."""
    import glide_run as G

    seen = np.zeros(3, dtype=np.int64)     # failures before retirement, inside it, of the terminal settlement
    for cls in SERVED:
        for scn in F.scenarios(oracle, cls):
            ora = F.oracle_run(oracle, scn, trajectories=True)
            ry = int(scn.cfgd["retirement_years"])
            got = G.integers(ora, ry)
            for k in G.INTEGERS:
                assert got[k].tolist() == ora[k].astype(np.uint64).tolist(), (k, scn.context("integers from columns"))
            b = ora["ruin_year_bins"].astype(np.int64)
            seen += [b[0], b[1:ry + 1].sum(), b[ry + 1]]
    assert seen[1] > 0, seen.tolist()
    print(f"failures before retirement / inside it / of the terminal settlement: {seen.tolist()}")
