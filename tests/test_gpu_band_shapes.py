"""The band (K3) and histogram (K2) kernels of csrc/mcr_aggregate.hip at the shapes the rest of the suite never reaches,
each against pandas / NumPy, bit for bit:

* rows longer than 2^24 entries (10-bit sub-histograms, the halved cell list, the largest LDS requests of the file), on
  one GPU and sharded over two ranks with n_local below and n_total above 2^24;
* every launch-geometry knob of the bracketed route ("results are exact for every value");
* more than 1 024 and more than 4 096 rows (one past each threshold of the counting pass's per-row grid);
* the generic slab kernel for every row (MCR_RQ_SLAB_LUT=0);
* K2's scalar path: values not 16-byte aligned and / or flags not 2-byte aligned.

A test here fails if a kernel returns a neighbouring order statistic or an off-by-one bin: there is no tolerance."""

from __future__ import annotations

import json
import os
import socket
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import aggregation as A
from rq_long_rows_dist_worker import LONG_N, NINE, SHARDED_ROWS, long_rows
from test_simulator_gpu import _random_row, _rows_for_bracket_test

pytestmark = pytest.mark.gpu

SEVEN = tuple(A.TRAJECTORY_QUANTILES)
FIFTEEN = tuple(float(q) for q in np.linspace(0.02, 0.98, 15))
EXTREME = (0.0, 1.0, 0.5, 0.999, 0.001)
LONG_SETS = {"seven": SEVEN, "nine": NINE, "fifteen": FIFTEEN, "extreme": EXTREME}
GEOMETRY_KNOBS = ("MCR_RQ_SLAB_WGS", "MCR_RQ_SAMPLE_WGS", "MCR_RQ_COLLECT_PER_ROW", "MCR_RQ_SAMPLE_DIV")


def _pandas_sets(rows: np.ndarray, sets: dict) -> dict:
    """``{name: [n_rows, len(qs)]}``: what the reference evaluates (simulation.py:1059-1113), ONE call over the union of all
    sets' q — a column of the result depends on its own q only, so this equals one call per set bit for bit."""
    union = sorted({float(q) for qs in sets.values() for q in qs})
    frame = pd.DataFrame(rows.T).quantile(union, axis=0).to_numpy()          # [len(union), n_rows]
    at = {q: i for i, q in enumerate(union)}
    return {name: np.ascontiguousarray(frame[[at[float(q)] for q in qs]].T) for name, qs in sets.items()}


def _valid_counts(rows: np.ndarray) -> list:
    return (~np.isnan(rows)).sum(axis=1).tolist()


def _assert_same_quantiles(got, exp, what):
    """Bit for bit, NaN == NaN, row by row (the message names the first rows that differ)."""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = [(r, got[r].tolist(), exp[r].tolist()) for r in range(exp.shape[0]) if not np.array_equal(got[r], exp[r], equal_nan=True)]
    assert not bad, (what, len(bad), bad[:3])


def _assert_same_histogram(got, edges, exp, exp_edges, what):
    assert got.tolist() == exp.tolist(), (what, got.tolist(), exp.tolist())
    assert np.array_equal(edges, exp_edges), (what, edges.tolist(), exp_edges.tolist())


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---- A / B: rows longer than 2^24 entries ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_host():
    """The 5 x (2^24 + 71) slab on the host (row stride n + 1: even, so the 16-byte loads run) and pandas' quantiles of all
    four sets, computed once.  No device work here: the sharded test starts its ranks before this process touches the GPU."""
    t0 = time.perf_counter()
    n = LONG_N
    host = np.full((5, n + 1), 123.0)
    host[:, :n] = long_rows()
    t1 = time.perf_counter()
    exp = _pandas_sets(host[:, :n], LONG_SETS)
    print(f"long rows: {n} entries x 5 rows generated in {t1 - t0:.1f} s, pandas in {time.perf_counter() - t1:.1f} s")
    return SimpleNamespace(n=n, host=host, exp=exp, valid=_valid_counts(host[:, :n]))


@pytest.fixture(scope="module")
def long_dev(long_host):
    import torch

    dev = torch.as_tensor(long_host.host, device="cuda")
    assert dev.data_ptr() % 16 == 0 and dev.stride(0) % 2 == 0
    yield dev
    del dev
    torch.cuda.empty_cache()


def test_long_rows_sharded_over_two_ranks(long_host, tmp_path):
    """world = 2 over gloo on the one GPU, rows 0, 1, 2 and 4 of the long slab: every shard is shorter than 2^24 entries and
    the row longer, so `mcr_row_quantiles_sharded` counts into 1 024 sub-bins per interval (from n_total) with candidate
    buffers sized from n_local.  Both ranks must return pandas' quantiles of the WHOLE rows for the 7- and the 9-quantile
    set, on the bracketed route (with the same fallback count on both ranks) and on the stepwise radix route
    (MCR_RQ_SHARDED_BRACKET_MIN_N = 2^40, set by the workers for their second pair of calls)."""
    out = str(tmp_path / "res")
    port = _free_port()
    env = {k: v for k, v in os.environ.items() if k not in GEOMETRY_KNOBS + ("MCR_RQ_SHARDED_BRACKET_MIN_N", "MCR_RQ_BRACKET_MIN_N")}
    procs = []
    for rank in range(2):
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(REPO, "tests", "rq_long_rows_dist_worker.py"), out],
            env=dict(env, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                     OMP_NUM_THREADS="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    failed = None
    for rank, p in enumerate(procs):
        try:
            stdout, _ = p.communicate(timeout=300)
            if p.returncode != 0:
                failed = (rank, p.returncode, stdout.decode()[-3000:])
        except subprocess.TimeoutExpired:
            failed = (rank, "timed out", "")
        if failed:
            break
    if failed:                      # one rank down: its peer waits in a collective for ever — end it, start nothing more
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.communicate()
        pytest.fail(f"rank {failed[0]}: {failed[1]}\n{failed[2]}")
    res = [np.load(f"{out}.{rank}.npz") for rank in range(2)]
    rows = list(SHARDED_ROWS)
    valid = [long_host.valid[r] for r in rows]
    for name in ("seven", "nine"):
        exp = long_host.exp[name][rows]
        fb = [int(r[f"bracket_{name}_fallback"]) for r in res]
        print(f"long rows sharded over 2 ranks, {name}: rows that fell back per rank {fb}")
        for rank, r in enumerate(res):
            _assert_same_quantiles(r[f"bracket_{name}_q"], exp, ("bracketed", name, rank))
            _assert_same_quantiles(r[f"radix_{name}_q"], exp, ("radix", name, rank))
            assert r[f"bracket_{name}_counts"].tolist() == r[f"radix_{name}_counts"].tolist() == valid, (name, rank)
        assert fb[0] == fb[1] and fb[0] >= 0, fb        # the bracketed route, the same rows dropped on every rank


@pytest.mark.parametrize("name", list(LONG_SETS))
def test_long_rows_equal_pandas(long_host, long_dev, name):
    """2^24 + 71 entries per row: `sub_bits2 = 10`, the cell list halved, `rq_collect_kernel` at 80 KB and (9 and 15
    quantiles) `rq_slab_kernel<32>` at up to 98 KB of dynamic LDS.  Every order statistic must be pandas'."""
    got, counts = A.row_quantiles(long_dev, long_host.n, LONG_SETS[name])
    n_fb = A.last_fallback_rows()
    print(f"long rows, full slab, {name}: {n_fb} of 5 rows fell back")
    _assert_same_quantiles(got, long_host.exp[name], name)
    assert counts.tolist() == long_host.valid
    assert n_fb >= 0                                   # the bracketed route was taken


def test_long_rows_are_decided_on_their_brackets(long_host, long_dev):
    """The radix fallback would hide a wrong bracket route, so on the three row kinds that
    test_bracketed_row_quantiles_at_the_default_threshold holds to no fallback at 2^22 entries (continuous, continuous with
    NaNs, constant) NO row may fall back at this length either, for 7 and for 9 quantiles."""
    for name in ("seven", "nine"):
        got, counts = A.row_quantiles(long_dev[0:3], long_host.n, LONG_SETS[name])
        n_fb = A.last_fallback_rows()
        print(f"long rows, rows 0-2, {name}: {n_fb} of 3 rows fell back")
        _assert_same_quantiles(got, long_host.exp[name][0:3], name)
        assert counts.tolist() == long_host.valid[0:3]
        assert n_fb == 0, (name, n_fb)


def test_long_rows_radix_route(long_host, long_dev, monkeypatch):
    """The full radix passes over the same slab (the route of every row the brackets cannot decide) above 2^24."""
    monkeypatch.setenv("MCR_RQ_BRACKET_MIN_N", str(2**40))
    for name, qs in LONG_SETS.items():
        got, counts = A.row_quantiles(long_dev, long_host.n, qs)
        assert A.last_fallback_rows() == -1
        _assert_same_quantiles(got, long_host.exp[name], name)
        assert counts.tolist() == long_host.valid


def test_long_rows_scalar_loads_on_an_even_stride(long_host, long_dev):
    """The view [:, 1:] over n - 1 entries: the stride stays even but the base is only 8-byte aligned, so every kernel of
    the route takes its scalar-load branch."""
    n = long_host.n - 1
    view = long_dev[:, 1:]
    assert view.data_ptr() % 16 == 8 and view.stride(0) % 2 == 0
    host = long_host.host[:, 1:1 + n]
    exp = _pandas_sets(host, {"seven": SEVEN})["seven"]
    got, counts = A.row_quantiles(view, n, SEVEN)
    n_fb = A.last_fallback_rows()
    print(f"long rows, view from entry 1, seven: {n_fb} of 5 rows fell back")
    _assert_same_quantiles(got, exp, "view")
    assert counts.tolist() == _valid_counts(host)
    assert n_fb >= 0


# ---- C: launch geometry ------------------------------------------------------------------------------------------------

GEOMETRY_SETS = {"seven": SEVEN, "nine": NINE, "three": (0.0, 1.0, 0.5)}
GEOMETRY_CASES = ([{"MCR_RQ_SLAB_WGS": v} for v in (1, 7, 100000)] + [{"MCR_RQ_SAMPLE_WGS": v} for v in (1, 100000)] +
                  [{"MCR_RQ_COLLECT_PER_ROW": v} for v in (1, 3, 16, 64)] + [{"MCR_RQ_SAMPLE_DIV": v} for v in (2, 3, 1000)] +
                  [{"MCR_RQ_SLAB_WGS": 1, "MCR_RQ_SAMPLE_WGS": 1, "MCR_RQ_COLLECT_PER_ROW": 1, "MCR_RQ_SAMPLE_DIV": 2}])


@pytest.fixture(scope="module")
def geometry_rows():
    """Per (n, stride): the 14 rows of `_rows_for_bracket_test` on host and device, pandas' quantiles of the three sets and
    the counts of the DEFAULT launch (bracketed route forced, no knob set) — all computed once."""
    import torch

    cache = {}

    def get(n, stride):
        if (n, stride) not in cache:
            rows = _rows_for_bracket_test(np.random.default_rng(n), n, stride)
            dev = torch.as_tensor(rows, device="cuda")
            default_counts = {}
            with pytest.MonkeyPatch.context() as mp:
                for k in GEOMETRY_KNOBS:
                    mp.delenv(k, raising=False)
                mp.setenv("MCR_RQ_BRACKET_MIN_N", "1")
                for name, qs in GEOMETRY_SETS.items():
                    default_counts[name] = A.row_quantiles(dev, n, qs)[1].tolist()
                    assert A.last_fallback_rows() >= 0
            cache[(n, stride)] = SimpleNamespace(dev=dev, exp=_pandas_sets(rows[:, :n], GEOMETRY_SETS), default_counts=default_counts,
                                                 valid=_valid_counts(rows[:, :n]))
        return cache[(n, stride)]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("knobs", GEOMETRY_CASES, ids=lambda k: "-".join(f"{n[7:]}={v}" for n, v in k.items()))
@pytest.mark.parametrize("n,stride", [(70_000, 70_001), (300_001, 300_032)])
def test_every_launch_geometry_is_exact(geometry_rows, n, stride, knobs, monkeypatch):
    """Workgroups per row of the slab and of the sample pass, workgroups per row of the candidate collection and the size of
    the second sample only change who counts what: whatever their values (one knob at a time, and all four at their
    smallest), the quantiles are pandas' and the counts the default launch's."""
    case = geometry_rows(n, stride)
    for k in GEOMETRY_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCR_RQ_BRACKET_MIN_N", "1")
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    for name, qs in GEOMETRY_SETS.items():
        got, counts = A.row_quantiles(case.dev, n, qs)
        assert A.last_fallback_rows() >= 0, (knobs, name)
        _assert_same_quantiles(got, case.exp[name], (knobs, name))
        assert counts.tolist() == case.default_counts[name] == case.valid, (knobs, name)


# ---- D: many rows ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route,n,stride", [("bracketed", 4096, 4096), ("bracketed", 12_289, 12_290), ("radix", 200, 256)])
@pytest.mark.parametrize("n_rows", [1025, 4097])
def test_many_rows(n_rows, route, n, stride, monkeypatch):
    """One row past each threshold of the counting pass's per-row grid (`4096 / n_rows`, `1024 / n_rows`, floors of 1 and
    2): 1 025 and 4 097 rows — a 341-year horizon already has more than 1 024 — through the bracketed route and through
    the radix passes.  A row of 4 096 entries is one workgroup's work whatever the grid allows; at 12 289 entries (four
    workgroups' worth, odd, even stride) the floors bind: 3 and 1 workgroups per row in the slab pass, 2 in the sample
    pass, each striding over the row more than once.  Rows: 61 draws of `_random_row`, cycled."""
    import torch

    rng = np.random.default_rng(20260225 + n)
    pool = [_random_row(rng, n) for _ in range(61)]
    rows = np.full((n_rows, stride), -7.0)
    for r in range(n_rows):
        rows[r, :n] = pool[r % len(pool)]
    exp = _pandas_sets(rows[:, :n], {"seven": SEVEN})["seven"]
    if route == "bracketed":
        monkeypatch.setenv("MCR_RQ_BRACKET_MIN_N", "1")
    else:
        monkeypatch.delenv("MCR_RQ_BRACKET_MIN_N", raising=False)
    dev = torch.as_tensor(rows, device="cuda")
    try:
        got, counts = A.row_quantiles(dev, n, SEVEN)
        n_fb = A.last_fallback_rows()
    finally:
        del dev
        torch.cuda.empty_cache()                       # the slab (134 MB at 4 097 x 4 096) and ~1 GB of scratch
    print(f"{n_rows} rows of {n}, {route} route: {n_fb} rows fell back")
    assert (n_fb >= 0) if route == "bracketed" else (n_fb == -1)
    _assert_same_quantiles(got, exp, (n_rows, route))
    assert counts.tolist() == _valid_counts(rows[:, :n])


# ---- E: the generic slab kernel ----------------------------------------------------------------------------------------

_GENERIC_SLAB_CHILD = r"""
import json, os, sys
repo = sys.argv[1]
sys.path[:0] = [repo, os.path.join(repo, "tests")]
import numpy as np
import pandas as pd
import torch
from monte_carlo_retirement_amd import aggregation as A
from test_simulator_gpu import _rows_for_bracket_test

n, stride = 300_001, 300_032
rows = _rows_for_bracket_test(np.random.default_rng(n), n, stride)
dev = torch.as_tensor(rows, device="cuda")
out = {}
for name, qs in json.loads(sys.argv[2]).items():
    got, counts = A.row_quantiles(dev, n, qs)
    exp = pd.DataFrame(rows[:, :n].T).quantile(list(qs), axis=0).T.to_numpy()
    out[name] = {"equal": bool(np.array_equal(got, exp, equal_nan=True)), "counts": counts.tolist(),
                 "fallback": A.last_fallback_rows(), "got": got.tolist()}
print("RESULT " + json.dumps(out))
"""


def test_generic_slab_kernel_for_every_row():
    """MCR_RQ_SLAB_LUT=0 (read once per process, hence a fresh child) sends every row of the slab pass through
    `rq_count_kernel<P, true>`, which by default only sees rows whose bounds do not fit the bucket table."""
    n, stride = 300_001, 300_032
    sets = {"seven": SEVEN, "nine": NINE}
    env = {k: v for k, v in os.environ.items() if k not in GEOMETRY_KNOBS}
    r = subprocess.run([sys.executable, "-c", _GENERIC_SLAB_CHILD, REPO, json.dumps(sets)], timeout=300, capture_output=True, text=True,
                       env=dict(env, MCR_RQ_SLAB_LUT="0", MCR_RQ_BRACKET_MIN_N="1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    res = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][len("RESULT "):])
    rows = _rows_for_bracket_test(np.random.default_rng(n), n, stride)
    exp = _pandas_sets(rows[:, :n], sets)
    for name in sets:
        print(f"generic slab kernel, {name}: {res[name]['fallback']} of 14 rows fell back")
        _assert_same_quantiles(np.array(res[name]["got"], dtype=np.float64), exp[name], name)
        assert res[name]["equal"], name
        assert res[name]["counts"] == _valid_counts(rows[:, :n])
        assert res[name]["fallback"] >= 0


# ---- F: K2 on misaligned inputs ----------------------------------------------------------------------------------------

def _k2_values(rng, kind, n, scale):
    """The value menu of test_success_histogram_random_inputs."""
    if kind == 0:
        return rng.lognormal(0, rng.uniform(0.1, 2.5), n) * scale
    if kind == 1:
        return np.where(rng.random(n) < rng.uniform(0, 0.9), 0.0, rng.lognormal(0, 1, n) * scale)     # ruined paths: exact zeros
    if kind == 2:
        return rng.integers(0, int(rng.integers(1, 50)), n).astype(float) * scale                      # values ON bin edges
    if kind == 3:
        return np.full(n, scale)                                                                       # degenerate range
    v = rng.uniform(0, scale, n)
    v[rng.integers(0, n, max(1, n // 10))] = v.max()                                                   # ties at the right edge
    return v


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 300_001])
def test_k2_scalar_path_on_misaligned_views(n):
    """`mcr_minmax_success` / `mcr_histogram_success` take pairs only when `values` is 16-byte and `success` 2-byte
    aligned; a C caller with one struct-of-arrays buffer and an odd n is neither on every other column.  Views that start
    at element 0 or 1 of n + 1 values and of n + 1 flags, all four combinations (one takes the pair-wise path, three the
    scalar one), must all equal `np.histogram(values[success], bins, range)`: counts identical, edges bit-equal."""
    import torch

    rng = np.random.default_rng(20260226 + n)
    for kind in range(5):
        scale = 10.0 ** rng.uniform(-9, 9)
        v = _k2_values(rng, kind, n, scale)
        given = (float(v.min() - rng.uniform(0.1, 1.0) * scale), float(v.max() + rng.uniform(0.1, 1.0) * scale))
        vbuf = [torch.zeros(n + 1, dtype=torch.float64, device="cuda") for _ in range(2)]
        for o in range(2):
            vbuf[o][o:o + n] = torch.as_tensor(v, device="cuda")
        for share in (0.0, 0.5, 1.0):
            ok = (rng.random(n) < share).astype(np.uint8)
            sel = v[ok.astype(bool)]
            obuf = [torch.zeros(n + 1, dtype=torch.uint8, device="cuda") for _ in range(2)]
            for o in range(2):
                obuf[o][o:o + n] = torch.as_tensor(ok, device="cuda")
            for bins in (1, 7, 100):
                for value_range in (None, given):
                    exp, exp_edges = np.histogram(sel, bins=bins, range=value_range)
                    for vo in range(2):
                        for oo in range(2):
                            vals, flags = vbuf[vo][vo:vo + n], obuf[oo][oo:oo + n]
                            assert vals.data_ptr() % 16 == 8 * vo and flags.data_ptr() % 2 == oo
                            got, edges = A.success_histogram(vals, flags, bins, value_range=value_range)
                            what = (n, kind, share, bins, value_range, vo, oo)
                            _assert_same_histogram(got, edges, exp, exp_edges, what)
                            if sel.size == 0:
                                assert not got.any(), what
