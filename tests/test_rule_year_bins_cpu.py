"""Yearly bins under a spending rule without a GPU: the two entry points in header, binding and library (ABI still v8), the new
struct as a C compiler lays it out, the host-side validation (every refusal names its field before a device is looked for), the
loud failure without a device, and the arithmetic of `SpendingBands` and of the longer `split_year_bins` vector."""

from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spending_rule_model as M
from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import aggregation as A
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.spending_rules import SPENDING_QUANTILES, SpendingBands, SpendingRule

SYMBOLS = ("mcr_run_rule_year_bins_rng", "mcr_run_rule_year_bins_host_rng")
WM, RY = 7, 30


@pytest.fixture(scope="module")
def lib():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    return N.load_library()


def test_header_binding_library_and_struct_layout(lib, tmp_path):
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert int(re.search(r"#define MCR_ABI_VERSION (\d+)", header).group(1)) == N.MCR_ABI_VERSION == 8
    assert lib.mcr_abi_version() == 8
    declared = set(re.findall(r"\b(mcr_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in SYMBOLS:
        assert name in declared and name in N.ABI_SYMBOLS and hasattr(lib, name), name
    T = N.McrRuleYearBins
    lines = ['printf("size %zu\\n", sizeof(mcr_rule_year_bins));']
    lines += [f'printf("{f} %zu\\n", offsetof(mcr_rule_year_bins, {f}));' for f, _ in T._fields_]
    lines += ['printf("others %zu %zu %zu\\n", sizeof(mcr_year_bins), sizeof(mcr_spending_rule), sizeof(mcr_rule_outputs));']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    seen = dict(line.split() for line in out[:-1])
    assert int(seen["size"]) == C.sizeof(T) == 32
    for f, _ in T._fields_:
        assert int(seen[f]) == getattr(T, f).offset, f
    # no existing struct changed size
    assert out[-1].split()[1:] == [str(C.sizeof(N.McrYearBins)), "48", "24"] and C.sizeof(N.McrOutputs) == 136


def _params(**over):
    cfg = dict(M.plan_config("realized", REPO, WM), monthly_expenses=M.LEVELS["realized", WM]["symmetric"])
    cfg.update(over)
    return params_from_config(Config(**cfg))


class Call:
    """One call of the host form with sentinel-filled tables; `run` returns (rc, message, whether every table is untouched)."""

    def __init__(self, lib):
        self.lib = lib

    def run(self, params=None, rng=None, rule=M.RULES["symmetric"], n_m=8, m_edges="default", null_m_edges=False, per_path=False,
            n_bins=16, hist=False, no_table=False, device_form=False):
        p = _params() if params is None else params
        sz = E.query_sizes(p, WM)
        T, ry = sz.trajectory_len, sz.retirement_years
        e, we = E.default_year_edges(n_bins), E.default_wr_edges(8)
        me = np.linspace(0.5, 1.5, max(n_m, 1) + 1) if isinstance(m_edges, str) else np.ascontiguousarray(m_edges, dtype=np.float64)
        tabs = [np.full((T, n_bins + 2), 7, dtype=np.uint64), np.full((T, n_bins + 2), 7, dtype=np.uint64),
                np.full((ry, 10), 7, dtype=np.uint64), np.full(n_bins + 2, 7, dtype=np.uint64),
                np.full((ry, max(n_m, 1) + 2), 7, dtype=np.uint64), np.full((ry, 4), 7, dtype=np.uint64), np.full(2, 7, dtype=np.uint64)]
        o = N.McrOutputs()
        o.counters = tabs[6].ctypes.data
        extra = np.zeros(64)
        hist_bins, hist_edges = np.full(4, 7, dtype=np.uint64), np.linspace(0.0, 1e6, 5)
        if per_path:
            o.final_balance = extra.ctypes.data
        if hist:
            o.hist_bins, o.hist_edges, o.hist_n_bins = hist_bins.ctypes.data, hist_edges.ctypes.data, 4
        y = N.McrYearBins()
        y.edges, y.n_bins, y.wr_edges, y.n_wr_bins = e.ctypes.data, n_bins, we.ctypes.data, 8
        y.trajectory_bins, y.real_trajectory_bins, y.wr_bins, y.final_success_bins = (t.ctypes.data for t in tabs[:4])
        r = N.McrRuleYearBins()
        r.m_edges, r.n_m_bins = (None if null_m_edges else me.ctypes.data), n_m
        r.multiplier_bins = None if no_table else tabs[4].ctypes.data
        r.year_counts = tabs[5].ctypes.data
        rec = N.McrSpendingRule(*rule)
        g = N.philox_rng(5) if rng is None else rng
        if device_form:
            rc = self.lib.mcr_run_rule_year_bins_rng(C.byref(p), C.byref(g), 1, 0, 8, WM, C.byref(rec), C.byref(o), C.byref(y), C.byref(r), 0, None)
        else:
            rc = self.lib.mcr_run_rule_year_bins_host_rng(C.byref(p), C.byref(g), 1, 0, 8, WM, C.byref(rec), C.byref(o), C.byref(y), C.byref(r), 0)
        untouched = all(np.all(t == 7) for t in tabs) and np.all(hist_bins == 7)
        return rc, N.last_error(), untouched


def test_validation_names_the_field_before_any_device_work(lib):
    """Every refusal below comes from the host-side checks: the same code and message with or without a GPU in the box, and
    every table keeps its sentinel."""
    call = Call(lib)
    good = M.RULES["symmetric"]
    many = dict(M.plan_config("realized", REPO, WM))
    many["other_income_streams"] = [{"name": f"s{k}", "monthly_amount_today": 100.0 + k, "start_at_age": 50.0 + k, "duration_years": None,
                                     "inflation_indexed": True, "tax_rate": 0.1} for k in range(17)]
    p17 = params_from_config(Config(**many))
    assert p17.n_streams == 17
    bad_edges = np.linspace(0.5, 1.5, 9)
    cases = [
        ("upper", dict(rule=(0.9,) + good[1:]), N.MCR_ERR_INVALID_ARG, "upper"),
        ("cut", dict(rule=good[:2] + (1.0,) + good[3:]), N.MCR_ERR_INVALID_ARG, "cut"),
        ("ceiling nan", dict(rule=good[:5] + (float("nan"),)), N.MCR_ERR_INVALID_ARG, "ceiling"),
        ("n_m_bins 0", dict(n_m=0), N.MCR_ERR_INVALID_ARG, "n_m_bins"),
        ("n_m_bins 513", dict(n_m=N.MCR_MAX_YEAR_BINS + 1), N.MCR_ERR_INVALID_ARG, "n_m_bins"),
        ("null m_edges", dict(null_m_edges=True), N.MCR_ERR_INVALID_ARG, "m_edges"),
        ("descending m_edges", dict(m_edges=bad_edges[::-1]), N.MCR_ERR_INVALID_ARG, "m_edges"),
        ("nan m_edges", dict(m_edges=np.where(np.arange(9) == 3, np.nan, bad_edges)), N.MCR_ERR_INVALID_ARG, "m_edges"),
        ("inf m_edges", dict(m_edges=np.where(np.arange(9) == 8, np.inf, bad_edges)), N.MCR_ERR_INVALID_ARG, "m_edges"),
        ("per-path pointer", dict(per_path=True), N.MCR_ERR_INVALID_ARG, "per-path"),
        ("NumPy stream", dict(rng=N.numpy_rng(12345)), N.MCR_ERR_UNSUPPORTED, "NumPy stream"),
        ("17 streams", dict(params=p17), N.MCR_ERR_UNSUPPORTED, "17 income streams"),
        ("hist_bins", dict(hist=True), N.MCR_ERR_UNSUPPORTED, "hist_bins"),
    ]
    for name, kw, code, word in cases:
        for device_form in ((False, True) if "m_edges" not in name or name == "null m_edges" else (False,)):
            rc, msg, untouched = call.run(device_form=device_form, **kw)
            assert rc == code and word in msg and untouched, (name, device_form, rc, msg, untouched)


def _child(code: str) -> str:
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_launch_without_a_device_fails_loudly(lib):
    """There is no CPU fallback: valid arguments without a HIP device give MCR_ERR_NO_DEVICE from both entry points.  (In a
    child process: a call that initialises the HIP runtime would hold the GPU open for the rest of the session.)  With a device,
    the same calls with no paths succeed."""
    out = _child("import ctypes as C, json\n"
                 "from monte_carlo_retirement_amd import Config, params_from_config\n"
                 "from monte_carlo_retirement_amd import _native as N\n"
                 "lib = N.load_library()\n"
                 "p = params_from_config(Config(**json.load(open('tests/golden/paths_injected.json'))[0]['cfg']))\n"
                 "rule, rng, o, y, r = N.McrSpendingRule(1.2, 0.8, 0.1, 0.1, 0.5, 1.5), N.philox_rng(1), N.McrOutputs(), N.McrYearBins(), N.McrRuleYearBins()\n"
                 "a = lib.mcr_run_rule_year_bins_rng(C.byref(p), C.byref(rng), 1, 0, 0, 12, C.byref(rule), C.byref(o), C.byref(y), C.byref(r), 0, None)\n"
                 "ma = N.last_error().replace(' ', '_') or '-'\n"
                 "b = lib.mcr_run_rule_year_bins_host_rng(C.byref(p), C.byref(rng), 1, 0, 0, 12, C.byref(rule), C.byref(o), C.byref(y), C.byref(r), 0)\n"
                 "mb = N.last_error().replace(' ', '_') or '-'\n"
                 "print(lib.mcr_device_count(), a, ma, b, mb)")
    devices, a, ma, b, mb = out.split()[-5:]
    if int(devices) > 0:
        assert int(a) == 0 and int(b) == 0, (ma, mb)
    else:
        for rc, msg in ((a, ma), (b, mb)):
            assert int(rc) == N.MCR_ERR_NO_DEVICE and "no_usable_HIP_device" in msg, (rc, msg)


def _cells(row, edges):
    row = np.asarray(row, dtype=np.float64)
    return np.concatenate(([np.count_nonzero(row < edges[0])], np.histogram(row, bins=edges)[0],
                           [np.count_nonzero(row > edges[-1])])).astype(np.uint64)


def test_spending_bands_arithmetic_on_a_hand_made_table(lib):
    edges = np.array([0.5, 0.75, 1.0, 1.0, 1.25, 1.5])
    rows = [np.array([0.5, 0.6, 0.8, 0.9, 1.0, 1.0, 1.0, 1.2, 1.4, 1.5]), np.full(7, 1.0), np.array([]), np.array([0.4, 0.45, 1.6])]
    bins = np.stack([_cells(r, edges) for r in rows])
    base = 4000.0
    b = SpendingBands(bins, edges, base)
    assert b.retirement_years == 4 and b.alive.tolist() == [10, 7, 0, 3] and b.quantiles == SPENDING_QUANTILES
    lo, hi, est = A.bands_from_bins(bins, edges, list(SPENDING_QUANTILES))
    for got, ref in ((b.lo, lo), (b.hi, hi), (b.estimate, est)):
        assert np.array_equal(got, ref * base, equal_nan=True)
    exact = np.quantile(rows[0], SPENDING_QUANTILES) * base
    assert np.all(b.lo[0] <= exact) and np.all(exact <= b.hi[0]) and np.all(b.lo[0] <= b.estimate[0]) and np.all(b.estimate[0] <= b.hi[0])
    # all mass on 1.0, an edge shared by a zero-width bin: np.histogram's cell is [1.0, 1.25)
    assert np.all(b.lo[1] == base) and np.all(b.hi[1] == 1.25 * base)
    assert np.all(np.isnan(b.estimate[2])) and np.all(np.isnan(b.lo[2]))                 # a year nobody begins
    assert b.lo[3, 0] == -np.inf and b.hi[3, -1] == np.inf                               # outside the edges
    years = b.years()
    assert [y["alive"] for y in years] == [10, 7, 0, 3] and years[2]["p50"] == {"estimate": None, "lo": None, "hi": None}
    assert years[0]["p50"]["lo"] <= years[0]["p50"]["estimate"] <= years[0]["p50"]["hi"] and set(years[0]) == {"year", "alive", "p5", "p25", "p50", "p75", "p95"}
    assert years[3]["p5"]["lo"] is None and years[3]["p95"]["hi"] is None
    with pytest.raises(ValueError):
        SpendingBands(bins[:, :-1], edges, base)
    with pytest.raises(ValueError):
        SpendingBands(bins, edges, -1.0)
    # the default edges: linear from floor to ceiling; the neutral rule's range is one point (zero-width bins, legal)
    sym = SpendingRule(*M.RULES["symmetric"])
    d = E.default_multiplier_edges(sym)
    assert d.shape == (65,) and d[0] == 0.5 and d[-1] == 1.5 and np.all(np.diff(d) > 0)
    z = E.default_multiplier_edges(SpendingRule.neutral(), 8)
    assert z.tolist() == [1.0] * 9 and E.year_edge_array(z, "m_edges").shape == (9,)
    assert E.default_multiplier_edges(sym.record(), 1).tolist() == [0.5, 1.5]
    for bad in (0, N.MCR_MAX_YEAR_BINS + 1):
        with pytest.raises(ValueError):
            E.default_multiplier_edges(sym, bad)


def test_split_year_bins_round_trips_with_and_without_the_rule_blocks():
    sz = E.query_sizes(_params(), WM)
    T, ry = sz.trajectory_len, sz.retirement_years
    nb, nw, nm = 5, 3, 4
    plain_words = 2 + ry + sz.ruin_bins + 2 * T * (nb + 2) + ry * (nw + 2) + (nb + 2)
    vec = np.arange(plain_words, dtype=np.int64)
    plain = E.split_year_bins(vec, sz, nb, nw)
    assert list(plain) == ["counters", "wr_obs_counts", "ruin_year_bins", "trajectory_bins", "real_trajectory_bins", "wr_bins", "final_success_bins"]
    assert np.array_equal(np.concatenate([v.reshape(-1) for v in plain.values()]), vec)
    assert plain["trajectory_bins"].shape == (T, nb + 2) and plain["wr_bins"].shape == (ry, nw + 2) and plain["final_success_bins"].shape == (nb + 2,)
    longer = np.arange(plain_words + ry * 4 + ry * (nm + 2), dtype=np.int64)
    ruled = E.split_year_bins(longer, sz, nb, nw, nm)
    assert list(ruled) == list(plain) + ["rule_year_counts", "multiplier_bins"]
    for k in plain:                                           # the plain layout is a prefix of the rule one
        assert np.array_equal(ruled[k], plain[k]), k
    assert ruled["rule_year_counts"].shape == (ry, N.MCR_RULE_N_COUNTS) and ruled["multiplier_bins"].shape == (ry, nm + 2)
    assert np.array_equal(np.concatenate([v.reshape(-1) for v in ruled.values()]), longer)
    assert ruled["multiplier_bins"].base is not None and int(ruled["multiplier_bins"][-1, -1]) == longer[-1]
    with pytest.raises(AssertionError):
        E.split_year_bins(longer, sz, nb, nw)
    with pytest.raises((AssertionError, ValueError)):          # (too short for the rule blocks)
        E.split_year_bins(vec, sz, nb, nw, nm)
