"""The MONTH FORMS of the count-only path kernel (csrc/mcr_device.h: kMonthEqualRates; DESIGN.md "month forms"): a compile-time
variant that leaves out the select of the seller's realized-gains rate when both assets carry the same one.  It claims to keep
every bit: whole launches are compared through MCR_K1_MONTH_FORM, full mask against 0, on counters, ruin-year bins,
withdrawal-rate observation counts and histogram bins.  The variants exist for unsplit count-only launches only, plain or
time-sliced; the knobs of tests/test_gpu_growth_forms.py pick those kernels at small sizes.

Also here: the income-stream records that pay nothing, which the host no longer hands to the kernel (derive_params) — a
scenario with such records around a paying non-indexed one against the CPU oracle, which keeps every record."""

from __future__ import annotations

import json
import os

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

pytestmark = pytest.mark.gpu

KNOB = "MCR_K1_MONTH_FORM"
KNOBS = (KNOB, "MCR_K1_GROWTH_FORM", "MCR_K1_SPLIT_MAX_WAVES", "MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS",
         "MCR_K1_SEGMENT_ORDER")
EDGES = np.geomspace(1.0, 1e13, 65)
PLAIN = {"MCR_K1_SPLIT_MAX_WAVES": "0", "MCR_K1_SEGMENTS": "0"}     # the unsplit whole-path kernel, whatever the size


def _config(**over):
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        return dict(json.load(fh), **over)


def _params(**over):
    return params_from_config(Config(**_config(**over)))


def _run(p, wm, n, begin, env):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        r = E.run_batch_host(p, 4242, 1, begin, n, wm, want_summary=False, want_trajectories=False, hist_edges=EDGES)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return np.concatenate([r["counters"], r["ruin_year_bins"], r["wr_obs_counts"], r["hist_bins"]]).astype(np.int64)


def _forms_agree(p, wm, n, begin, env, what):
    assert E.month_form(p, wm) == 1, what                    # the launch's own choice is the full mask
    own = _run(p, wm, n, begin, env)
    assert int(own[1]) == n, what
    full = _run(p, wm, n, begin, dict(env, **{KNOB: "1"}))
    general = _run(p, wm, n, begin, dict(env, **{KNOB: "0"}))
    assert np.array_equal(full, own), (what, np.nonzero(full != own)[0][:8].tolist())
    assert np.array_equal(general, own), (what, np.nonzero(general != own)[0][:8].tolist())
    return own


def _sliced_paths():
    """The smallest launch that slices: one path block more than the resident slots (6 workgroups per CU)."""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 6 * 256 + 1


SLICED = {"MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENTS": "2", "MCR_K1_SEGMENT_ORDER": "0,1"}   # (the order: an error unless it slices)


def test_plain_launch_both_forms_give_the_same_integers():
    own = _forms_agree(_params(), 233, 20_000, 0, PLAIN, "config.json plain")
    assert 0 < int(own[0]) < 20_000


def test_time_sliced_launch_both_forms_give_the_same_integers():
    n = _sliced_paths()
    sliced = _forms_agree(_params(), 233, n, 5, SLICED, "config.json time-sliced")
    plain = _run(_params(), 233, n, 5, dict(PLAIN, **{KNOB: "0"}))
    assert np.array_equal(sliced, plain)


def test_time_sliced_launch_with_a_wave_that_straddles_2_to_the_32():
    _forms_agree(_params(), 233, _sliced_paths(), 2**32 - 100, SLICED, "time-sliced, straddling wave")


def test_time_sliced_launch_successors_first():
    """Segment 1's piece goes out before segment 0's: every successor recomputes its block from month 0 (no hand-over)."""
    n = _sliced_paths()
    env = dict(SLICED, MCR_K1_SEGMENT_ORDER="1,0", MCR_K1_SEGMENT_POLLS="1")
    swapped = _forms_agree(_params(), 233, n, 5, env, "time-sliced, order 1,0")
    assert np.array_equal(swapped, _run(_params(), 233, n, 5, dict(SLICED, **{KNOB: "0"})))


@pytest.mark.parametrize("wm", [0, 7])
def test_no_accumulation_and_a_partial_first_year(wm):
    _forms_agree(_params(), wm, 20_000, 0, PLAIN, f"wm = {wm}")


def test_unequal_rates_run_the_general_month_and_the_knob_is_an_error():
    p = _params(inv2_realized_gains_tax_rate=0.15)
    assert E.month_form(p, 233) == 0
    own = _run(p, 233, 20_000, 0, PLAIN)
    assert np.array_equal(_run(p, 233, 20_000, 0, dict(PLAIN, **{KNOB: "0"})), own)
    with pytest.raises(RuntimeError, match=KNOB):
        _run(p, 233, 20_000, 0, dict(PLAIN, **{KNOB: "1"}))
    with pytest.raises(RuntimeError, match=KNOB):            # 2 000 paths: the producer / consumer kernel has no variants
        _run(_params(), 233, 2_000, 0, {KNOB: "1"})


def _stream(amount, indexed=False, start=40.0, years=35):
    return {"name": f"s{amount}", "monthly_amount_today": amount, "start_at_age": start, "duration_years": years,
            "inflation_indexed": indexed, "tax_rate": 0.2}


MIXED = [_stream(0.0), _stream(1500.0), _stream(0.0, indexed=True), _stream(0.0, start=70.0, years=10)]


def test_a_paying_frozen_stream_beside_zero_ones_both_forms():
    p = _params(other_income_streams=MIXED)
    assert E.kept_streams(p, 233) == [(1, 0)]
    with_zeros = _forms_agree(p, 233, 20_000, 0, PLAIN, "frozen stream beside zero ones")
    without = _run(_params(other_income_streams=[MIXED[1]]), 233, 20_000, 0, PLAIN)
    assert np.array_equal(with_zeros, without)
    assert not np.array_equal(with_zeros, _run(_params(other_income_streams=[]), 233, 20_000, 0, PLAIN))   # (the stream matters)


def test_a_paying_frozen_stream_beside_zero_ones_against_the_oracle():
    """The oracle is handed every record, the zero ones included, with the lock slots of the full list."""
    from oracle import oracle as O

    p = _params(other_income_streams=MIXED)
    n = 2048
    gpu = E.run_batch_host(p, 12345, 1, 0, n, 233)
    cpu = O.run_batch(p, 12345, 1, 0, n, 233)
    assert np.array_equal(gpu["success"], cpu["success"])
    assert gpu["counters"].tolist() == cpu["counters"].tolist()
    np.testing.assert_allclose(gpu["final_balance"], cpu["final_balance"], rtol=1e-9, atol=1e-6)
