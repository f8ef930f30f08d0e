"""Yearly bins without a device: `aggregation.bands_from_bins` brackets the pandas / linear quantile of the binned data by
construction, the edge builders validate, and header, binding and struct agree (ABI still v8, mcr_outputs still 17 x 8)."""

from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import aggregation as A
from monte_carlo_retirement_amd import engine as E

QS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)


def _cells(row, edges):
    """The kernel's row layout from per-path values: below | np.histogram | above."""
    row = np.asarray(row, dtype=np.float64)
    return np.concatenate(([np.count_nonzero(row < edges[0])], np.histogram(row, bins=edges)[0],
                           [np.count_nonzero(row > edges[-1])])).astype(np.uint64)


@pytest.mark.parametrize("n", [1, 2, 7, 10_001])
def test_brackets_contain_the_quantile(n):
    rng = np.random.default_rng(100 + n)
    edges = E.default_year_edges(64)
    rows = []
    for _ in range(4):
        x = rng.lognormal(13.0, 1.5, n)
        x[rng.random(n) < 0.3] = 0.0                       # 30 % exact zeros (failed paths)
        rows.append(x)
    bins = np.stack([_cells(x, edges) for x in rows])
    assert bins.sum(axis=1).tolist() == [n] * 4
    lo, hi, est = A.bands_from_bins(bins, edges, QS)
    assert lo.shape == hi.shape == est.shape == (4, len(QS))
    for r, x in enumerate(rows):
        exact = np.quantile(x, QS)
        assert np.all(lo[r] <= exact) and np.all(exact <= hi[r]), (lo[r], exact, hi[r])
        assert np.all(lo[r] <= est[r]) and np.all(est[r] <= hi[r])
        assert np.all(np.isfinite(est[r]))


def test_below_above_empty_and_zero_width():
    edges = np.array([10.0, 20.0, 20.0, 20.0, 40.0, 80.0])    # two zero-width bins
    x = np.array([1.0, 2.0, 15.0, 20.0, 20.0, 20.0, 30.0, 50.0, 500.0, 900.0])
    bins = np.stack([_cells(x, edges), np.zeros(edges.size + 1, dtype=np.uint64), _cells([20.0] * 5, edges)])
    lo, hi, est = A.bands_from_bins(bins, edges, QS)
    exact = np.quantile(x, QS)
    assert np.all(lo[0] <= exact) and np.all(exact <= hi[0])
    assert lo[0, 0] == -np.inf and np.isnan(est[0, 0])          # the minimum is in the below cell
    assert hi[0, -1] == np.inf and np.isnan(est[0, -1])         # the maximum in the above cell
    assert np.isfinite(lo[0, 3]) and np.isfinite(hi[0, 3]) and lo[0, 3] <= est[0, 3] <= hi[0, 3]
    assert np.all(np.isnan(lo[1])) and np.all(np.isnan(hi[1])) and np.all(np.isnan(est[1]))   # empty row
    # all mass on an edge shared by zero-width bins: np.histogram puts it into the last of them, [20, 40)
    assert np.all(lo[2] == 20.0) and np.all(hi[2] == 40.0)
    # a 1-D row is one row
    lo1, hi1, _ = A.bands_from_bins(bins[0], edges, [0.5])
    assert lo1.shape == (1, 1) and lo1[0, 0] == lo[0, 3] and hi1[0, 0] == hi[0, 3]
    with pytest.raises(ValueError):
        A.bands_from_bins(bins[:, :-1], edges, QS)
    with pytest.raises(ValueError):
        A.bands_from_bins(bins, edges[::-1], QS)
    with pytest.raises(ValueError):
        A.bands_from_bins(bins, edges, [1.5])


def test_edge_builders_validate():
    e = E.default_year_edges(64)
    assert e.shape == (65,) and e[0] == 0.0 and e[1] == 1.0 and np.all(np.diff(e) > 0) and np.isclose(e[-1], 1e12)
    assert E.default_year_edges(N.MCR_MAX_YEAR_BINS).shape == (N.MCR_MAX_YEAR_BINS + 1,)
    w = E.default_wr_edges(50)
    assert w.shape == (51,) and w[0] == 0.0 and w[-1] == 100.0
    for bad in (1, 0, -3, N.MCR_MAX_YEAR_BINS + 1):
        with pytest.raises(ValueError):
            E.default_year_edges(bad)
    for bad in (0, -1, N.MCR_MAX_YEAR_BINS + 1):
        with pytest.raises(ValueError):
            E.default_wr_edges(bad)
    with pytest.raises(ValueError):
        E.default_year_edges(64, lo=0.0)
    with pytest.raises(ValueError):
        E.default_wr_edges(10, hi=float("inf"))
    for bad in ([1.0], [3.0, 2.0], [0.0, float("nan")], [0.0, float("inf")], np.arange(N.MCR_MAX_YEAR_BINS + 2.0)):
        with pytest.raises(ValueError):
            E.year_edge_array(bad)
    assert E.year_edge_array([0, 1, 1, 2]).dtype == np.float64        # equal neighbours are allowed


def test_header_binding_and_struct_layout(tmp_path):
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert int(re.search(r"#define MCR_ABI_VERSION (\d+)", header).group(1)) == N.MCR_ABI_VERSION == 8
    assert C.sizeof(N.McrOutputs) == 136
    assert int(re.search(r"#define MCR_MAX_YEAR_BINS (\d+)", header).group(1)) == N.MCR_MAX_YEAR_BINS >= 256
    declared = set(re.findall(r"\b(mcr_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in ("mcr_run_year_bins_rng", "mcr_run_year_bins_host_rng", "mcr_run_year_bins_multi_host_rng"):
        assert name in declared and name in N.ABI_SYMBOLS, name
    # the mcr_year_bins layout as gcc sees it
    T = N.McrYearBins
    lines = ['printf("size %zu\\n", sizeof(mcr_year_bins));']
    lines += [f'printf("{f} %zu\\n", offsetof(mcr_year_bins, {f}));' for f, _ in T._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    seen = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(seen["size"]) == C.sizeof(T)
    for f, _ in T._fields_:
        assert int(seen[f]) == getattr(T, f).offset, f
