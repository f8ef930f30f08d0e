"""The STREAM FORM of the count-only path kernel (csrc/mcr_device.h: kStreamsInRegs; DESIGN.md "stream form") and the scalar
month counters of the same kernels (the running row, the month of the year, the next priority threshold).

The stream form keeps at most two inflation-indexed income-stream records in registers for the whole launch and issues their
FMAs in list order; it claims to keep every bit.  Whole launches are compared through MCR_K1_STREAM_FORM, mask 1 against 0, on
counters, ruin-year bins, withdrawal-rate observation counts and histogram bins, and their counts against the CPU oracle.  Each
case's monthly_expenses is calibrated with the oracle alone (bisection on the success count, as tests/count_fuzz.py does), so
that successes and failures both occur; a case the oracle leaves all-or-nothing is redrawn on another path range.

The scalar counters run in form 0 as well: launches at working months of every alignment to the year, with contribution growth
on, are held to the oracle's integers.  The variants exist for unsplit count-only launches only, plain or time-sliced; the knobs
of tests/test_gpu_month_forms.py pick those kernels at small sizes."""

from __future__ import annotations

import functools
import json
import math
import os

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

pytestmark = pytest.mark.gpu

KNOB = "MCR_K1_STREAM_FORM"
KNOBS = (KNOB, "MCR_K1_MONTH_FORM", "MCR_K1_GROWTH_FORM", "MCR_K1_SPLIT_MAX_WAVES", "MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS",
         "MCR_K1_SEGMENT_POLLS", "MCR_K1_SEGMENT_ORDER")
EDGES = np.geomspace(1.0, 1e13, 65)
PLAIN = {"MCR_K1_SPLIT_MAX_WAVES": "0", "MCR_K1_SEGMENTS": "0"}     # the unsplit whole-path kernel, whatever the size
SEED, STREAM = 4242, 1
COUNT_KEYS = ("counters", "ruin_year_bins", "wr_obs_counts")
CAL_LO, CAL_HI, CAL_STEPS, REDRAWS = 50.0, 2.0e6, 14, 6


def _config(**over):
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        return dict(json.load(fh), **over)


def _stream(amount, start, years=None, indexed=True, tax=0.2):
    return {"name": f"s{amount}", "monthly_amount_today": amount, "start_at_age": start, "duration_years": years,
            "inflation_indexed": indexed, "tax_rate": tax}


# retirement begins at 40 + wm / 12: wm = 240 -> 60.0, wm = 233 -> 59.42
A, B = _stream(3000.0, 62.0), _stream(1200.0, 65.0, years=5, tax=0.1)
#        name                                   config overrides                                                        wm   paths
CASES = [
    ("config.json 512",                         {},                                                                     233, 512),
    ("config.json 321",                         {},                                                                     233, 321),
    ("opens at retirement month 0",             {"retirement_years": 12, "other_income_streams": [_stream(2500.0, 60.0)]},       240, 512),
    ("opens mid-year",                          {"retirement_years": 12, "other_income_streams": [_stream(2500.0, 63.0)]},       233, 512),
    ("opens before retirement",                 {"retirement_years": 12, "other_income_streams": [_stream(2500.0, 50.0)]},       233, 384),
    ("closes mid-horizon",                      {"retirement_years": 12, "other_income_streams": [_stream(2500.0, 61.0, 6)]},    233, 512),
    ("opens after the horizon",                 {"retirement_years": 12, "other_income_streams": [_stream(2500.0, 80.0)]},       233, 256),
    ("two overlapping records, A then B",       {"retirement_years": 12, "other_income_streams": [A, B]},               233, 512),
    ("two overlapping records, B then A",       {"retirement_years": 12, "other_income_streams": [B, A]},               233, 512),
    ("no record",                               {"retirement_years": 12, "other_income_streams": []},                   233, 300),
]
THREE = {"retirement_years": 12, "other_income_streams": [A, B, _stream(500.0, 64.0)]}
WM_ALIGNMENT = [0, 1, 5, 11, 12, 13, 23]


def _oracle():
    from oracle import oracle as O

    return O


def _oracle_counts(cfgd, wm, n, begin):
    r = _oracle().run_batch(params_from_config(Config(**cfgd)), SEED, STREAM, begin, n, wm, want_trajectories=False)
    return {k: np.asarray(r[k]).astype(np.int64) for k in COUNT_KEYS}


def calibrate(cfgd, wm, n):
    """(config with its monthly_expenses calibrated, first path, the oracle's counts): bisection in log-spending on the oracle's
    success count over the case's own paths, towards half of them failing; redrawn on the next path range while the oracle
    leaves the case all-or-nothing."""
    for draw in range(REDRAWS):
        begin = 1000 * draw
        lo, hi = math.log(CAL_LO), math.log(CAL_HI)
        for _ in range(CAL_STEPS):
            mid = 0.5 * (lo + hi)
            c = _oracle_counts(dict(cfgd, monthly_expenses=math.exp(mid)), wm, n, begin)["counters"]
            if 2 * int(c[0]) < n:
                hi = mid        # more than half fail: spend less
            else:
                lo = mid
        cal = dict(cfgd, monthly_expenses=round(math.exp(0.5 * (lo + hi)), 2))
        counts = _oracle_counts(cal, wm, n, begin)
        if 0 < int(counts["counters"][0]) < n:
            return cal, begin, counts
    raise AssertionError(f"the oracle leaves {cfgd.get('other_income_streams')} at wm = {wm} all-or-nothing on {REDRAWS} path ranges")


@functools.lru_cache(maxsize=None)
def calibrated_case(i):
    name, over, wm, n = CASES[i]
    return calibrate(_config(**over), wm, n)


@functools.lru_cache(maxsize=None)
def calibrated_alignment(wm):
    years = 3 + WM_ALIGNMENT.index(wm) % 3                       # 3, 4, 5 retirement years
    cfgd = _config(retirement_years=years, other_income_streams=[_stream(2500.0, 42.5)])
    assert cfgd["contribution_growth_rate_annual"] > 0.0
    return calibrate(cfgd, wm, 448)


def _run(p, wm, n, begin, env):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return E.run_batch_host(p, SEED, STREAM, begin, n, wm, want_summary=False, want_trajectories=False, hist_edges=EDGES)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _ints(r):
    return np.concatenate([r["counters"], r["ruin_year_bins"], r["wr_obs_counts"], r["hist_bins"]]).astype(np.int64)


def _equals_the_oracle(r, counts, what):
    for k in COUNT_KEYS:
        got = np.asarray(r[k]).astype(np.int64)
        assert np.array_equal(got, counts[k]), (what, k, got.tolist(), counts[k].tolist())


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_stream_form_1_equals_form_0_and_the_oracle(i):
    name, _, wm, n = CASES[i]
    cfgd, begin, counts = calibrated_case(i)
    p = params_from_config(Config(**cfgd))
    assert E.stream_form(p, wm) == 1, name                       # the launch's own choice is the full mask
    own = _run(p, wm, n, begin, PLAIN)
    regs = _run(p, wm, n, begin, dict(PLAIN, **{KNOB: "1"}))
    loop = _run(p, wm, n, begin, dict(PLAIN, **{KNOB: "0"}))
    assert int(own["counters"][1]) == n and 0 < int(own["counters"][0]) < n, name
    assert np.array_equal(_ints(regs), _ints(own)), (name, np.nonzero(_ints(regs) != _ints(own))[0][:8].tolist())
    assert np.array_equal(_ints(loop), _ints(own)), (name, np.nonzero(_ints(loop) != _ints(own))[0][:8].tolist())
    _equals_the_oracle(own, counts, name)
    _equals_the_oracle(loop, counts, name)


def test_the_two_list_orders_are_the_same_plan():
    """(What the pair of order cases rests on: the same records, the same calibration target; the records overlap in years 5-10.)"""
    a, b = CASES[7][1]["other_income_streams"], CASES[8][1]["other_income_streams"]
    assert a == b[::-1] and a[0]["monthly_amount_today"] != a[1]["monthly_amount_today"]


def test_three_indexed_records_run_the_list_and_the_knob_is_an_error():
    cfgd, begin, counts = calibrate(_config(**THREE), 233, 512)
    p = params_from_config(Config(**cfgd))
    assert E.stream_form(p, 233) == 0
    own = _run(p, 233, 512, begin, PLAIN)
    assert np.array_equal(_ints(_run(p, 233, 512, begin, dict(PLAIN, **{KNOB: "0"}))), _ints(own))
    _equals_the_oracle(own, counts, "three records")
    with pytest.raises(RuntimeError, match=KNOB):
        _run(p, 233, 512, begin, dict(PLAIN, **{KNOB: "1"}))


def test_the_knob_on_a_kernel_without_variants_is_an_error():
    p = params_from_config(Config(**_config()))
    with pytest.raises(RuntimeError, match=KNOB):                # 512 paths, no other knob: the producer / consumer kernel
        _run(p, 233, 512, 0, {KNOB: "1"})
    _run(p, 233, 512, 0, {KNOB: "0"})                            # (mask 0 is every kernel's own)


@pytest.mark.parametrize("wm", WM_ALIGNMENT)
def test_working_months_of_every_alignment_equal_the_oracle(wm):
    """The accumulation's month-of-year counter (contribution growth in month 13, 25, ...; the year's sample in month 12, 24, ...)
    and the retirement year's end at mi = 11 - wm % 12, in both stream forms."""
    cfgd, begin, counts = calibrated_alignment(wm)
    p = params_from_config(Config(**cfgd))
    for env in (PLAIN, dict(PLAIN, **{KNOB: "0"})):
        r = _run(p, wm, 448, begin, env)
        assert 0 < int(r["counters"][0]) < 448
        _equals_the_oracle(r, counts, (wm, env.get(KNOB)))


def _sliced_paths():
    """The smallest launch that slices: one path block more than the resident slots (6 workgroups per CU)."""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 6 * 256 + 1


@pytest.mark.parametrize("order,polls", [("0,1", None), ("1,0", "1")], ids=["default order", "successors first"])
def test_time_sliced_window_opens_in_a_later_segment(order, polls):
    """Two segments cut config.json's 50 retirement years at year 17; the pension opens in year 25, inside segment 1, which takes
    the row over from its predecessor (default order) or recomputes the block from month 0 (its piece goes out first)."""
    n = _sliced_paths()
    cfgd = _config(other_income_streams=[_stream(4000.0, 40.0 + 233 / 12.0 + 25.5, tax=0.275)])
    p = params_from_config(Config(**cfgd))
    assert E.stream_form(p, 233) == 1
    env = {"MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENTS": "2", "MCR_K1_SEGMENT_ORDER": order}
    if polls is not None:
        env["MCR_K1_SEGMENT_POLLS"] = polls
    sliced = _ints(_run(p, 233, n, 5, env))
    plain = _ints(_run(p, 233, n, 5, dict(PLAIN, **{KNOB: "0"})))
    assert int(plain[1]) == n and 0 < int(plain[0]) < n
    assert np.array_equal(sliced, plain), np.nonzero(sliced != plain)[0][:8].tolist()
