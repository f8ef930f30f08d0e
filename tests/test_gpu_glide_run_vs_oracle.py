"""The glide whole-path launches (`mcr_run_glide_rng` in its summary form, `mcr_run_glide_year_bins_host_rng`) against the CPU
oracle's model of a glide path, on the stratified random plans of tests/count_fuzz.py under the five tables of tests/glide_fuzz.py.

The unmodified oracle cannot run a glide path; tests/glide_model.cpp is its path loop over its own exported steps with the weight
of the row, and tests/test_glide_model_cpu.py holds that model to the oracle bit for bit under constant tables.  Here the model's
per-path columns and yearly trajectories are the reference of every plan of the six classes the glide launches serve:

* the summary columns through `same_summary` of tests/test_gpu_numpy_stream_vs_oracle.py (flags and integers exactly, money within
  the path contract of tests/test_gpu_differential.py); the model keeps no integers, so they are formed from its columns
  (tests/glide_run.py: `integers`, held to the oracle's own by tests/test_glide_run_cpu.py);
* the four yearly tables through `same_year_bins` of the same file: the rule of tests/bin_rule.py, under which the model's rows of
  these plans have two entries near an edge in all (tests/test_glide_run_cpu.py pins it).

No tolerance is new and no plan is waived: identical outcomes are demanded below the 2^33 money scale, so each model run's scale
is asserted.  Printed per class: the worst error of the summary columns relative to max(|ref|, the path's money scale), and how
many table cells moved under the rule.  Measured on an MI355X with the suite's seed (LABNOTES R41)."""

from __future__ import annotations

import numpy as np
import pytest

import count_fuzz as F
import glide_fuzz as GF
import glide_run as G
from monte_carlo_retirement_amd import engine as E
from test_gpu_count_routes_vs_oracle import _env
from test_gpu_numpy_stream_vs_oracle import SUMMARY, same_summary, same_year_bins, year_bin_rows

pytestmark = pytest.mark.gpu
CLASSES = tuple(c for c in F.CLASSES if c != "generic")
_MOVED = {}          # class -> table cells moved under the bin rule: summed over the classes run so far


def _ctx(scn, route):
    return scn.context(f"{route}; Philox stream")


def _worst_scaled(got, ref, keys) -> float:
    scale = np.maximum(1.0, np.abs(ref["trajectory"]).max(axis=0))
    return max(float(np.max(np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), scale))) for k in keys)


def _moved(got, ref) -> int:
    import bin_rule

    total = 0
    for name, data, edges in year_bin_rows(got, ref):
        table = got[name].astype(np.int64).reshape(data.shape[0], -1)
        total += sum(bin_rule.row_verdict(table[t], row, edges)[0] for t, row in enumerate(data))
    return total


@pytest.mark.parametrize("cls", CLASSES)
def test_glide_launches_equal_the_model(oracle, cls):
    worst, moved, runs_seen = 0.0, 0, 0
    try:
        for scn, runs in GF.class_runs(oracle, cls):
            p, at, ry = scn.params(), (scn.seed, scn.stream, scn.begin, scn.n), int(scn.cfgd["retirement_years"])
            for name, table, run in zip(GF.NAMES, GF.tables(scn), runs):
                route = f"glide launch under table {name} = {table}"
                assert F.money_scale(run) < F.SCALE_LIMIT, _ctx(scn, route + ": money scale")
                ref = G.with_integers(run, ry)
                with _env({}):
                    summary = E.run_glide_host(p, *at, scn.wm, table, want="summary")
                    bins = E.run_glide_year_bins_host(p, *at, scn.wm, table)
                worst = max(worst, _worst_scaled(summary, ref, SUMMARY))
                same_summary(scn, summary, ref, route + " (MODE 1)", ctx=_ctx)
                same_year_bins(scn, bins, ref, route + " (MODE 3)", ctx=_ctx)
                moved += _moved(bins, ref)
                runs_seen += 1
    finally:
        print(f"glide launches {cls}: worst summary error against the model relative to max(|ref|, the path's money scale) {worst:.3e}, "
              f"{moved} table cells moved under the bin rule ({runs_seen} runs)")
    # two yearly samples near an edge in the whole suite (tests/test_glide_run_cpu.py): at most four moved cells over ALL classes.
    # (The sum is over the classes run so far in this process: it is the bound of the issue when the whole file runs in one process;
    #  under -k or a distributed runner it holds for the classes seen.  same_year_bins above is the check of every row either way.)
    _MOVED[cls] = moved
    assert sum(_MOVED.values()) <= 4, _MOVED
