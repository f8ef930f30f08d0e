"""The joint income probe (`mcr_probe_income_joint_rng`) against the CPU oracle, on the stratified random plans of
tests/count_fuzz.py and the five income options of tests/test_gpu_income_vs_oracle.py.

tests/test_gpu_joint_outcomes.py compares the masks with plain launches of the same library; an error both share passes it.
Here the ORACLE's own per-path `success` columns of a plan's five options give ``F @ F.T`` and the {all, none} counts, and the
GPU's matrix, extremes and masks must equal them exactly, for every plan of every class.  As there, identical flags are demanded
only below the 2^33 money scale, so each oracle run's scale is asserted; no plan is waived."""

from __future__ import annotations

import numpy as np
import pytest

import count_fuzz as F
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from test_gpu_income_vs_oracle import class_runs
from test_gpu_joint_outcomes import expected, unpack

pytestmark = pytest.mark.gpu
STREAM_FIELDS = ("monthly_amount_today", "start_at_age", "duration_years")


def oracle_flags(runs, k):
    return np.stack([np.asarray(run["success"]).astype(np.uint8) for run in runs[5 * k: 5 * k + 5]])


@pytest.mark.parametrize("cls", F.CLASSES)
def test_joint_income_probe_equals_the_oracle(oracle, cls, monkeypatch):
    monkeypatch.delenv("MCR_INCOME_FANOUT_MIN_WAVES", raising=False)
    lib = N.load_library()
    plans, runs = class_runs(oracle, cls)
    assert plans, cls
    for k, (scn, (idx, opts, _)) in enumerate(plans):
        for o, run in zip(opts, runs[5 * k: 5 * k + 5]):
            assert F.money_scale(run) < F.SCALE_LIMIT, (o, scn.context("joint income probe"))
        flags = oracle_flags(runs, k)
        assert flags.shape == (5, scn.n)
        own = scn.cfgd["other_income_streams"][idx]
        money = (scn.cfgd["initial_balance"], scn.cfgd["monthly_contribution"], scn.cfgd["monthly_expenses"])
        records = [money + tuple(o.get(f, own[f]) for f in STREAM_FIELDS) for o in opts]
        counts, joint, extremes, masks = E.probe_income_joint(scn.params(), scn.seed, scn.stream, scn.begin, scn.n, scn.wm, idx, records)
        launches = lib.mcr_probe_income_last_fanout_launches()
        want_joint, want_extremes = expected(flags)
        assert joint.cpu().numpy().tolist() == want_joint.tolist(), (idx, opts, scn.context("joint income probe"))
        assert extremes.cpu().numpy().tolist() == want_extremes, scn.context("joint income probe")
        got, tail = unpack(masks, scn.n)
        assert np.array_equal(got, flags) and not tail.any(), scn.context("joint income probe")
        assert counts.cpu().numpy().tolist() == [[int(c), scn.n] for c in want_joint.diagonal()]
        if cls == "generic":     # 17 or more paying streams, or the exact month: one launch per option
            assert launches == 0, scn.context("joint income probe")
        else:
            assert launches >= 1, scn.context("joint income probe")


def test_the_options_disagree_on_paths(oracle):
    """The comparison above is not vacuous: over all classes at least a quarter of the option pairs have a discordant path,
    one on which one option succeeds and the other fails (the reference alone: 206 of 610 pairs with the suite's seed)."""
    discordant = total = 0
    for cls in F.CLASSES:
        plans, runs = class_runs(oracle, cls)
        for k in range(len(plans)):
            flags = oracle_flags(runs, k)
            for a in range(5):
                for b in range(a + 1, 5):
                    discordant += bool((flags[a] != flags[b]).any())
                    total += 1
    assert total > 0 and 4 * discordant >= total, (discordant, total)
