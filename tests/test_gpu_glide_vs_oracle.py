"""The glide OUTCOME and JOINT probes (`mcr_probe_glide_paths_{outcomes,joint}_rng`) against the CPU oracle's model of a glide
path, on the stratified random plans of tests/count_fuzz.py and the options of tests/glide_fuzz.py.

The unmodified oracle cannot run a glide path; tests/glide_model.cpp is its path loop over its own exported steps with the
weight of the row, and tests/test_glide_model_cpu.py holds that model to the oracle bit for bit under constant tables.  Here the
model's per-path columns of every option are the reference, for every plan of the six classes the glide fan-out serves, with the
comparisons of tests/test_gpu_allocation_vs_oracle.py: the NaN pattern of both rows and `years_to_ruin` exactly, `final_balance`
within the path contract of tests/test_gpu_differential.py (``ABS + REL x max(|c|, the path's money scale)``, imported), the
ruin-month counts of the GPU's rows equal to the counts of the model's columns, the counts equal; and for the joint form the
matrix and extremes of ``expected(flags)`` of the model's `success` columns, the masks unpacking to those columns with clean
tails.  Identical outcomes are demanded only below the 2^33 money scale, so each model run's scale is asserted; no plan is
waived.  Every call reports at least one glide fan-out launch.

The `generic` class (17 or more paying streams, or the exact month) has no route under a glide path: every call returns
MCR_ERR_UNSUPPORTED and leaves every output untouched."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import count_fuzz as F
import glide_fuzz as GF
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from test_gpu_count_routes_vs_oracle import _env
from test_gpu_differential import ABS, REL
from test_gpu_joint_outcomes import expected, unpack
from test_gpu_option_outcomes_vs_oracle import month_counts

pytestmark = pytest.mark.gpu
CLASSES = tuple(c for c in F.CLASSES if c != "generic")


def _route(ctx):
    launches = N.load_library().mcr_probe_glide_paths_last_fanout_launches()
    assert launches >= 1, (launches, ctx)


def _usable_runs(scn, runs):
    for name, run in zip(GF.NAMES, runs):
        assert F.money_scale(run) < F.SCALE_LIMIT, (name, scn.context("glide paths: money scale"))


@pytest.mark.parametrize("cls", CLASSES)
def test_outcome_probe_equals_the_model(oracle, cls):
    worst = 0.0
    for scn, runs in GF.class_runs(oracle, cls):
        ctx = scn.context(f"glide outcomes probe, options {GF.NAMES} = {GF.tables(scn)}")
        _usable_runs(scn, runs)
        want_fin, want_ruin, scale = GF.oracle_rows(runs)
        L = len(runs)
        assert want_fin.shape == want_ruin.shape == scale.shape == (L, scn.n)
        with _env({}):
            counts, fin_t, ruin_t = E.probe_glide_paths_outcomes(scn.params(), scn.seed, scn.stream, scn.begin, scn.n, scn.wm, GF.records(scn))
            _route(ctx)
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
    print(f"glide paths {cls}: worst final-balance error relative to max(|ref|, the path's money scale) {worst:.3e}")


@pytest.mark.parametrize("cls", CLASSES)
def test_joint_probe_equals_the_model(oracle, cls):
    for scn, runs in GF.class_runs(oracle, cls):
        ctx = scn.context(f"glide joint probe, options {GF.NAMES} = {GF.tables(scn)}")
        _usable_runs(scn, runs)
        flags = GF.oracle_flags(runs)
        assert flags.shape == (len(runs), scn.n)
        with _env({}):
            counts, joint, extremes, masks = E.probe_glide_paths_joint(scn.params(), scn.seed, scn.stream, scn.begin, scn.n, scn.wm, GF.records(scn))
            _route(ctx)
        want_joint, want_extremes = expected(flags)
        assert joint.cpu().numpy().tolist() == want_joint.tolist(), ctx
        assert extremes.cpu().numpy().tolist() == want_extremes, ctx
        got, tail = unpack(masks, scn.n)
        assert np.array_equal(got, flags), ([int(k) for k in np.flatnonzero((got != flags).any(axis=1))], ctx)
        assert not tail.any(), ctx
        assert counts.cpu().numpy().tolist() == [[int(c), scn.n] for c in want_joint.diagonal()], ctx


def test_the_generic_class_is_unsupported_and_touches_nothing(oracle):
    import torch

    lib = N.load_library()
    stream = torch.cuda.current_stream(0).cuda_stream
    sentinel, fsentinel = -0x1234_5678, -12345.678
    for scn in F.scenarios(oracle, "generic"):
        ctx = scn.context("glide probes, generic class")
        (table, n_table, arr), L = E._glide_option_records(GF.records(scn))
        p, rng = scn.params(), N.philox_rng(scn.seed)
        counts = torch.full((L, 2), sentinel, dtype=torch.int64, device="cuda")
        masks = torch.full((L, 16), sentinel, dtype=torch.int64, device="cuda")
        joint = torch.full((L, L), sentinel, dtype=torch.int64, device="cuda")
        extremes = torch.full((2,), sentinel, dtype=torch.int64, device="cuda")
        fin = torch.full((L, 1024), fsentinel, dtype=torch.float64, device="cuda")
        ruin = torch.full((L, 1024), fsentinel, dtype=torch.float64, device="cuda")
        rows = N.McrOptionOutcomes(fin.data_ptr(), ruin.data_ptr(), 1024)
        head = (C.byref(p), C.byref(rng), scn.stream, scn.begin, scn.n, scn.wm, table, n_table, arr, L, C.c_void_p(counts.data_ptr()))
        with _env({}):
            for rc in (lib.mcr_probe_glide_paths_rng(*head, 0, C.c_void_p(stream)),
                       lib.mcr_probe_glide_paths_joint_rng(*head, C.c_void_p(masks.data_ptr()), C.c_void_p(joint.data_ptr()),
                                                           C.c_void_p(extremes.data_ptr()), 0, C.c_void_p(stream)),
                       lib.mcr_probe_glide_paths_outcomes_rng(*head, C.byref(rows), 0, C.c_void_p(stream))):
                assert rc == N.MCR_ERR_UNSUPPORTED, (rc, N.last_error(), ctx)
                assert "not supported under a glide path" in N.last_error(), (N.last_error(), ctx)
                assert lib.mcr_probe_glide_paths_last_fanout_launches() == 0
        torch.cuda.synchronize()
        for t in (counts, masks, joint, extremes):
            assert (t.cpu() == sentinel).all(), ctx
        assert (fin.cpu() == fsentinel).all() and (ruin.cpu() == fsentinel).all(), ctx
