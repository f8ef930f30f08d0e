"""The allocation OUTCOME and JOINT probes (`mcr_probe_allocations_{outcomes,joint}_rng`) against the CPU oracle, on the
stratified random plans of tests/count_fuzz.py and the options of tests/allocation_fuzz.py.

tests/test_gpu_allocation_probe.py compares these probes with summary and plain launches of the same library.  Here the
unmodified ORACLE's own per-path columns of every option (an allocation option is a `Config` override) are the reference, for
every plan of all seven classes, with the comparisons tests/test_gpu_probe_options_vs_oracle.py makes for the scenario and
assumption families: the NaN pattern of both rows and `years_to_ruin` exactly, `final_balance` within the path contract of
tests/test_gpu_differential.py (``ABS + REL x max(|c|, the path's money scale)``, imported), the ruin-month counts of the GPU's
rows equal to the counts of the oracle's columns, the counts equal; and for the joint form the matrix and extremes of
``expected(flags)`` of the oracle's `success` columns, the masks unpacking to those columns with clean tails.  Identical outcomes
are demanded only below the 2^33 money scale, so each oracle run's scale is asserted; no plan is waived.
tests/test_allocation_fuzz_cpu.py shows from the oracle alone that the options move paths.

The route: the family reports its fan-out launches (0 for the `generic` class, whose plans have 17 or more paying streams or the
exact month: one launch per option; at least 1 otherwise)."""

from __future__ import annotations

import numpy as np
import pytest

import allocation_fuzz as AF
import count_fuzz as F
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from test_gpu_count_routes_vs_oracle import _env
from test_gpu_differential import ABS, REL
from test_gpu_joint_outcomes import expected, unpack
from test_gpu_option_outcomes_vs_oracle import month_counts

pytestmark = pytest.mark.gpu


def _route(cls, ctx):
    launches = N.load_library().mcr_probe_allocations_last_fanout_launches()
    assert (launches == 0) if cls == "generic" else (launches >= 1), (launches, ctx)


def _usable_runs(scn, runs):
    for name, run in zip(AF.NAMES, runs):
        assert F.money_scale(run) < F.SCALE_LIMIT, (name, scn.context("allocations: money scale"))


@pytest.mark.parametrize("cls", F.CLASSES)
def test_outcome_probe_equals_the_oracle(oracle, cls):
    worst = 0.0
    for scn, runs in AF.class_runs(oracle, cls):
        ctx = scn.context(f"allocation outcomes probe, options {AF.NAMES} = {AF.splits(scn)}")
        _usable_runs(scn, runs)
        want_fin, want_ruin, scale = AF.oracle_rows(runs)
        L = len(runs)
        assert want_fin.shape == want_ruin.shape == scale.shape == (L, scn.n)
        with _env({}):
            counts, fin_t, ruin_t = E.probe_allocations_outcomes(scn.params(), scn.seed, scn.stream, scn.begin, scn.n, scn.wm, AF.records(scn))
            _route(cls, ctx)
            ry = int(scn.cfgd["retirement_years"])
            months = E.ruin_month_counts(ruin_t, scn.n, ry).cpu().numpy()
        fin, ruin = fin_t.cpu().numpy()[:, :scn.n], ruin_t.cpu().numpy()[:, :scn.n]
        assert np.array_equal(np.isnan(fin), np.isnan(want_fin)) and np.array_equal(np.isnan(ruin), np.isnan(want_ruin)), ctx
        assert np.array_equal(np.isnan(ruin), ~np.isnan(fin)), ctx
        np.testing.assert_allclose(ruin, want_ruin, rtol=0, atol=0, equal_nan=True, err_msg=ctx)
        ok = ~np.isnan(want_fin)
        err = np.abs(fin[ok] - want_fin[ok])
        bound = np.maximum(np.abs(want_fin[ok]), scale[ok])
        worst = max(worst, float((err / bound).max()) if err.size else 0.0)
        assert np.all(err <= ABS + REL * bound), (ctx, float(err.max()))
        assert months.tolist() == month_counts(want_ruin, ry).tolist(), ctx
        assert counts.cpu().numpy().tolist() == [[int(c), scn.n] for c in ok.sum(axis=1)], ctx
    print(f"allocations {cls}: worst final-balance error relative to max(|ref|, the path's money scale) {worst:.3e}")


@pytest.mark.parametrize("cls", F.CLASSES)
def test_joint_probe_equals_the_oracle(oracle, cls):
    for scn, runs in AF.class_runs(oracle, cls):
        ctx = scn.context(f"allocation joint probe, options {AF.NAMES} = {AF.splits(scn)}")
        _usable_runs(scn, runs)
        flags = AF.oracle_flags(runs)
        assert flags.shape == (len(runs), scn.n)
        with _env({}):
            counts, joint, extremes, masks = E.probe_allocations_joint(scn.params(), scn.seed, scn.stream, scn.begin, scn.n, scn.wm, AF.records(scn))
            _route(cls, ctx)
        want_joint, want_extremes = expected(flags)
        assert joint.cpu().numpy().tolist() == want_joint.tolist(), ctx
        assert extremes.cpu().numpy().tolist() == want_extremes, ctx
        got, tail = unpack(masks, scn.n)
        assert np.array_equal(got, flags), ([int(k) for k in np.flatnonzero((got != flags).any(axis=1))], ctx)
        assert not tail.any(), ctx
        assert counts.cpu().numpy().tolist() == [[int(c), scn.n] for c in want_joint.diagonal()], ctx
