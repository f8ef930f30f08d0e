"""The SCREENED count-only route (csrc/mcr_screen.h: screen_kernel + path_kernel's LIST form) against the CPU oracle, and
screen_kernel's own per-path values against a plain fp64 restatement of its month, on the random qualifying plans of
tests/count_fuzz.py (`screened_scenarios`: five tax bases x eight plans x two expense levels; 0-2 indexed income records with
windows that open before retirement, never open or never close, contribution growth, rho = +-1, 20-60 % volatility, rates near
1, odd month counts, path ranges at 2^32 - 100 and 2^40, 1025 / 705 paths).  tests/test_screen_fuzz_cpu.py shows on the CPU
that the plans qualify, that the restatement (tests/screen_model.py) reproduces the oracle on every path it calls SAFE, and that
the plans are not vacuous.

Counts: under MCR_K1_SCREEN=1 with the 256-path re-run, the unsplit re-run (MCR_K1_SCREEN_EXPECTED=1e6) and the 64-path re-run
(MCR_K1_RERUN_PRODUCERS=2), `counters`, `wr_obs_counts` and `ruin_year_bins` equal the oracle's exactly, and the classic
route's (MCR_K1_SCREEN=0), so that a failure names the half at fault.

Why the counts are not enough: SAFE needs 24 months of need in hand, so a kernel that computed the need several times too small
(a misplaced income window, a dropped contribution-growth step) would still call SAFE only paths that succeed, and every count
would pass.  Classification (`engine.screen_paths`, the kernel alone): the class equals the model's on every path whose
decisive margin `slack` is further than the plan's tolerance from 1; every kernel-SAFE path succeeds in the oracle with no ruin
year; on the paths SAFE in both, `min_ratio` and `final_total` are within the tolerance of the fp64 model's (`min_ratio` inf in
both where no month had a need); the lowest kernel `min_ratio` among SAFE keeps the margin.  DOUBTFUL lanes are not compared on
the two values: they stop when their whole wave is doubtful, so what they hold depends on their neighbours.  The tolerance is
the plan's own, max(2e-4, 8 x the deviation of the model's float32 run from its fp64 run), at most 1e-2: measured from the
reference, never from the kernel (count_fuzz.screen_reference).

Edge plans (allocation 0 or 1, initial balance 0): every path DOUBTFUL, and the counts still the oracle's: the full-list re-run
at a ragged size, in all three forms.

Observed on MI355X: the table in LABNOTES.md ("screened route vs oracle")."""

from __future__ import annotations

import os
from contextlib import contextmanager

import numpy as np
import pytest

import count_fuzz as F
from monte_carlo_retirement_amd import engine as E

pytestmark = pytest.mark.gpu

COUNT_KEYS = ("counters", "wr_obs_counts", "ruin_year_bins")
RERUNS = {"256-path re-run": {}, "unsplit re-run": {"MCR_K1_SCREEN_EXPECTED": "1e6"}, "64-path re-run": {"MCR_K1_RERUN_PRODUCERS": "2"}}
KEPT_MARGIN = 24.0 * (1.0 - 1e-5)       # cap x rcp(need) against cap >= 24 need: an fp32 rounding apart (tests/test_gpu_screen.py)


@contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in F.SCREEN_KNOBS}
    for k in F.SCREEN_KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _ints(r):
    return np.concatenate([np.asarray(r[k]).astype(np.int64) for k in COUNT_KEYS])


def _count_only(scn, p, env, screened):
    with _env(env):
        assert E.screen(p, scn.wm, scn.n) == screened, scn.context("route", env)
        return _ints(E.run_batch_host(p, scn.seed, scn.stream, scn.begin, scn.n, scn.wm, want_summary=False, want_trajectories=False))


def _same_counts(scn, level, p, ora):
    want = _ints(ora)
    classic = _count_only(scn, p, {"MCR_K1_SCREEN": "0"}, False)
    assert int(classic[1]) == scn.n
    assert np.array_equal(classic, want), ("classic route vs oracle", np.nonzero(classic != want)[0][:8].tolist(), scn.context(level))
    for name, env in RERUNS.items():
        env = dict(env, MCR_K1_SCREEN="1")
        got = _count_only(scn, p, env, True)
        where = np.nonzero(got != want)[0][:8].tolist()
        assert np.array_equal(got, classic), ("screened route vs classic route", name, where, got[:2].tolist(), classic[:2].tolist(), scn.context(level, env))
        assert np.array_equal(got, want), ("screened route vs oracle", name, where, scn.context(level, env))


def _rel(got, want):
    return np.abs(got.astype(np.float64) / want - 1.0)


def _same_classification(scn, level, p, ora, ref, edge):
    """screen_kernel alone on plan `scn`: the comparisons of the module's docstring.  Returns the figures of the plan's row."""
    m, tol = ref["fp64"], ref["tol"]
    with _env({}):
        k = E.screen_paths(p, scn.seed, scn.stream, scn.begin, scn.n, scn.wm)
    assert set(np.unique(k["cls"]).tolist()) <= {0, 1}, scn.context(level)
    safe = k["cls"] == 0
    decided = np.abs(m["slack"] - 1.0) > tol
    wrong = decided & (safe != m["safe"])
    both = safe & m["safe"]
    no_need = np.isinf(m["min_ratio"][both])
    d_ratio = d_total = 0.0
    if both.any():
        d_total = float(_rel(k["final_total"][both], m["final_total"][both]).max())
        if not no_need.all():
            d_ratio = float(_rel(k["min_ratio"][both][~no_need], m["min_ratio"][both][~no_need]).max())
    low = float(k["min_ratio"][safe].min()) if safe.any() else float("inf")
    row = {"paths": scn.n, "model_safe": int(m["safe"].sum()), "kernel_safe": int(safe.sum()), "excused": int((~decided).sum()),
           "differ": int((~decided & (safe != m["safe"])).sum()), "tol": tol, "d_ratio": d_ratio, "d_total": d_total}
    print(f"  {scn.cfgd['scenario']} {level}: {scn.n} paths, SAFE model {row['model_safe']} kernel {row['kernel_safe']}, excused by slack "
          f"{row['excused']} (classes differ on {row['differ']}), tol {tol:.2e} (dev {ref['dev']:.2e}), "
          f"max dev min_ratio {d_ratio:.2e} final_total {d_total:.2e}, lowest min_ratio among SAFE {low:.3f}")
    assert not wrong.any(), ("class", np.nonzero(wrong)[0][:8].tolist(), m["slack"][wrong][:8].tolist(), scn.context(level))
    assert np.all(ora["success"][safe] == 1) and np.all(np.isnan(ora["years_to_ruin"][safe])), \
        ("SAFE but no success", np.nonzero(safe & (ora["success"] == 0))[0][:8].tolist(), scn.context(level))
    assert np.array_equal(np.isinf(k["min_ratio"][both]), no_need), ("min_ratio: months with a need", scn.context(level))
    assert d_ratio <= tol, ("min_ratio", d_ratio, tol, scn.context(level))
    assert d_total <= tol, ("final_total", d_total, tol, scn.context(level))
    assert low >= KEPT_MARGIN, (low, scn.context(level))
    if edge is not None:
        assert not safe.any(), (edge, int(safe.sum()), scn.context(level))
    return row


@pytest.mark.parametrize("level", list(F.SCREENED_LEVELS))
@pytest.mark.parametrize("base", F.SCREENED_BASES)
def test_screened_route_and_screening_kernel_equal_the_oracle_and_the_model(oracle, base, level):
    plans = F.screened_scenarios(oracle, base)
    F.oracle_runs(oracle, [((F.at_level(s, level),), {}) for s in plans])
    rows = []
    for s in plans:
        scn = F.at_level(s, level)
        p = scn.params()
        ora = F.oracle_run(oracle, scn)
        ref = F.screen_reference(s, level)
        assert ref["tol"] <= F.SCREENED_TOL_MAX, scn.context(level)
        _same_counts(scn, level, p, ora)
        row = _same_classification(scn, level, p, ora, ref, F.screened_edge(s))
        if F.screened_edge(s) is None:
            rows.append(row)
    total = lambda key: sum(r[key] for r in rows)       # noqa: E731
    most = lambda key: max(r[key] for r in rows)        # noqa: E731
    paths = total("paths")
    print(f"{base} {level}: interior paths {paths}, SAFE share model {total('model_safe') / paths:.3f} kernel {total('kernel_safe') / paths:.3f}, "
          f"excused by slack {total('excused')} (classes differ on {total('differ')}), largest tol {most('tol'):.2e}, "
          f"largest dev min_ratio {most('d_ratio'):.2e} final_total {most('d_total'):.2e}")
