"""The host's choice of a launch's STREAM FORM (csrc/mcr_hip.hip: stream_form_of; DESIGN.md "stream form"), through
mcr_k1_stream_form — no device needed.

Bit 0 (streams in registers): the records the path kernel is given — other_income_streams without the ones that pay nothing —
are at most two, none beyond the by-value block, every one inflation-indexed, and the launch pays no annual-gains tax.  The
knob MCR_K1_STREAM_FORM forces a lower mask only.  Its third error, a non-zero mask on a launch whose kernel has no variants,
needs a launch: tests/test_gpu_stream_forms.py."""

from __future__ import annotations

import json
import os

import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

KNOB = "MCR_K1_STREAM_FORM"


@pytest.fixture(autouse=True)
def _no_knob():
    old = os.environ.pop(KNOB, None)
    yield
    os.environ.pop(KNOB, None)
    if old is not None:
        os.environ[KNOB] = old


def _scenario(name="config.json", **over):
    with open(os.path.join(REPO, "scenarios", name)) as fh:
        return Config(**dict(json.load(fh), **over))


def _stream(amount, indexed=True, start=40.0, years=35):
    return {"name": f"s{amount}", "monthly_amount_today": amount, "start_at_age": start, "duration_years": years,
            "inflation_indexed": indexed, "tax_rate": 0.2}


def _form(streams, wm=233, **over):
    return E.stream_form(params_from_config(_scenario(other_income_streams=streams, **over)), wm)


def test_shipped_scenarios_keep_their_pension_in_registers():
    assert E.stream_form(params_from_config(_scenario()), 233) == 1
    assert E.stream_form(params_from_config(_scenario("jorge.json")), 75) == 1
    assert E.stream_form(params_from_config(_scenario()), 0) == 1


def test_an_empty_list_qualifies():
    assert _form([]) == 1


def test_one_and_two_indexed_records_qualify():
    assert _form([_stream(800.0)]) == 1
    assert _form([_stream(800.0), _stream(300.0, start=70.0, years=None)]) == 1


def test_records_that_pay_nothing_do_not_count():
    zeros = [_stream(0.0, indexed=False), _stream(0.0), _stream(0.0, indexed=False)]
    assert _form(zeros) == 1                                                 # nothing is kept: the empty list
    assert _form([zeros[0], _stream(800.0), zeros[1], _stream(300.0), zeros[2]]) == 1
    assert _form([_stream(0.0, indexed=False)] * 20 + [_stream(800.0)]) == 1   # 21 records, one kept: nothing in the extra table


def test_three_indexed_records_do_not_qualify():
    assert _form([_stream(800.0), _stream(300.0), _stream(100.0)]) == 0


def test_a_paying_frozen_record_does_not_qualify():
    assert _form([_stream(800.0, indexed=False)]) == 0
    assert _form([_stream(800.0), _stream(1.0, indexed=False)]) == 0
    assert _form([_stream(1.0, indexed=False), _stream(800.0)]) == 0


def test_a_list_beyond_the_inline_block_does_not_qualify():
    assert _form([_stream(10.0 + i) for i in range(17)]) == 0


def test_an_annual_gains_tax_does_not_qualify():
    assert _form([_stream(800.0)], inv1_use_realized_gains_tax_system=False, inv1_annual_tax_on_gains_rate=0.2) == 0
    # (an annual rate on an asset that uses the realized system is not applied at all)
    assert _form([_stream(800.0)], inv1_annual_tax_on_gains_rate=0.2) == 1


def test_rates_that_need_the_exact_month_do_not_qualify():
    assert _form([_stream(800.0)], inv1_realized_gains_tax_rate=1.0, inv2_realized_gains_tax_rate=1.0) == 0


def test_the_knob_forces_a_lower_mask_only():
    two = params_from_config(_scenario())
    three = params_from_config(_scenario(other_income_streams=[_stream(800.0), _stream(300.0), _stream(100.0)]))
    for want in (0, 1):
        os.environ[KNOB] = str(want)
        assert E.stream_form(two, 233) == want
    os.environ[KNOB] = "0"
    assert E.stream_form(three, 233) == 0
    os.environ[KNOB] = "1"
    with pytest.raises(ValueError, match=KNOB):                             # three records: the bit is not available
        E.stream_form(three, 233)
    for junk in ("2", "3", "-1", "x", "1x"):                                # not a stream form / not a number
        os.environ[KNOB] = junk
        with pytest.raises(ValueError, match=KNOB):
            E.stream_form(two, 233)


def test_the_other_forms_of_the_headline_launch_are_what_they_were():
    p = params_from_config(_scenario())
    assert E.month_form(p, 233) == 1
    assert E.growth_form(p, 233) == 3
    os.environ[KNOB] = "0"                                                   # (the knobs are independent)
    assert E.month_form(p, 233) == 1
    assert E.growth_form(p, 233) == 3
