"""The scenario and assumption OUTCOME and JOINT probes (`mcr_probe_{scenarios,assumptions}_{outcomes,joint}_rng`) against the CPU
oracle, on the stratified random plans of tests/count_fuzz.py and the options of tests/option_fuzz.py.

tests/test_gpu_option_outcomes.py and tests/test_gpu_joint_outcomes.py compare these probes with summary and plain launches of
the same library; only the income family was held to the oracle (tests/test_gpu_option_outcomes_vs_oracle.py,
tests/test_gpu_joint_vs_oracle.py).  Here the ORACLE's own per-path columns of every option are the reference, for every plan
of every class, with the comparisons the income family has: the NaN pattern of both rows and `years_to_ruin` exactly,
`final_balance` within the path contract of tests/test_gpu_differential.py (``ABS + REL x max(|c|, the path's money scale)``,
imported), the ruin-month counts of the GPU's rows equal to the counts of the oracle's columns, the counts equal; and for the
joint form the matrix and extremes of ``expected(flags)`` of the oracle's `success` columns, the masks unpacking to those columns
with clean tails.  Identical outcomes are demanded only below the 2^33 money scale, so each oracle run's scale is asserted; no
plan is waived.  tests/test_option_fuzz_cpu.py shows from the oracle alone that the options move paths.

The route: the assumption family reports its fan-out launches (0 for the `generic` class, whose plans have 17 or more paying
streams or the exact month: one launch per option; at least 1 otherwise); the scenario family has no such counter."""

from __future__ import annotations

import numpy as np
import pytest

import count_fuzz as F
import option_fuzz as OF
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.stress import assumption_records
from test_gpu_count_routes_vs_oracle import _env
from test_gpu_differential import ABS, REL
from test_gpu_joint_outcomes import expected, unpack
from test_gpu_option_outcomes_vs_oracle import month_counts

pytestmark = pytest.mark.gpu


def _records(scn, family):
    if family == "scenarios":
        return OF.triples(scn)
    return assumption_records(scn.config(), OF.overrides(scn, "assumptions"))


def _route(cls, family, ctx):
    """The assumption family's fan-out launch counter after a probe call; nothing to read for the scenario family."""
    if family != "assumptions":
        return
    launches = N.load_library().mcr_probe_assumptions_last_fanout_launches()
    assert (launches == 0) if cls == "generic" else (launches >= 1), (launches, ctx)


def _usable_runs(scn, family, runs):
    for name, run in zip(OF.NAMES[family], runs):
        assert F.money_scale(run) < F.SCALE_LIMIT, (name, scn.context(f"{family}: money scale"))


@pytest.mark.parametrize("cls", F.CLASSES)
@pytest.mark.parametrize("family", OF.FAMILIES)
def test_outcome_probes_equal_the_oracle(oracle, family, cls):
    probe = {"scenarios": E.probe_scenarios_outcomes, "assumptions": E.probe_assumptions_outcomes}[family]
    worst = 0.0
    for scn, runs in OF.class_runs(oracle, cls, family):
        ctx = scn.context(f"{family} outcomes probe, options {OF.NAMES[family]}")
        _usable_runs(scn, family, runs)
        want_fin, want_ruin, scale = OF.oracle_rows(runs)
        L = len(runs)
        assert want_fin.shape == want_ruin.shape == scale.shape == (L, scn.n)
        with _env({}):
            counts, fin_t, ruin_t = probe(scn.params(), scn.seed, scn.stream, scn.begin, scn.n, scn.wm, _records(scn, family))
            _route(cls, family, ctx)
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
    print(f"{family} {cls}: worst final-balance error relative to max(|ref|, the path's money scale) {worst:.3e}")


@pytest.mark.parametrize("cls", F.CLASSES)
@pytest.mark.parametrize("family", OF.FAMILIES)
def test_joint_probes_equal_the_oracle(oracle, family, cls):
    probe = {"scenarios": E.probe_scenarios_joint, "assumptions": E.probe_assumptions_joint}[family]
    for scn, runs in OF.class_runs(oracle, cls, family):
        ctx = scn.context(f"{family} joint probe, options {OF.NAMES[family]}")
        _usable_runs(scn, family, runs)
        flags = OF.oracle_flags(runs)
        assert flags.shape == (len(runs), scn.n)
        with _env({}):
            counts, joint, extremes, masks = probe(scn.params(), scn.seed, scn.stream, scn.begin, scn.n, scn.wm, _records(scn, family))
            _route(cls, family, ctx)
        want_joint, want_extremes = expected(flags)
        assert joint.cpu().numpy().tolist() == want_joint.tolist(), ctx
        assert extremes.cpu().numpy().tolist() == want_extremes, ctx
        got, tail = unpack(masks, scn.n)
        assert np.array_equal(got, flags), ([int(k) for k in np.flatnonzero((got != flags).any(axis=1))], ctx)
        assert not tail.any(), ctx
        assert counts.cpu().numpy().tolist() == [[int(c), scn.n] for c in want_joint.diagonal()], ctx
