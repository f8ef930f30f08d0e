"""The host's choice of a launch's MONTH FORM (csrc/mcr_hip.hip: month_form_of; DESIGN.md "month forms"), through
mcr_k1_month_form, and the list of income-stream records the path kernel is given (derive_params, through
mcr_k1_kept_streams) — no device needed.

Bit 0 (equal realized-gains rates): both assets use the realized-gains system with the SAME non-zero rate, and neither pays an
annual-gains tax.  A record of other_income_streams whose monthly_amount_today is 0 pays an exact zero in every month: the
kernel does not get it, and the lock slots of the non-indexed streams are numbered over the records that are kept."""

from __future__ import annotations

import json
import os

import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

KNOB = "MCR_K1_MONTH_FORM"


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


def _stream(amount, indexed, start=40.0, years=35):
    return {"name": f"s{amount}", "monthly_amount_today": amount, "start_at_age": start, "duration_years": years,
            "inflation_indexed": indexed, "tax_rate": 0.2}


def test_shipped_scenarios_have_equal_rates():
    assert E.month_form(params_from_config(_scenario()), 233) == 1
    assert E.month_form(params_from_config(_scenario("jorge.json")), 75) == 1
    assert E.month_form(params_from_config(_scenario()), 0) == 1            # (the bit does not depend on the accumulation)


def test_unequal_rates_do_not_qualify():
    p = params_from_config(_scenario(inv2_realized_gains_tax_rate=0.15))
    assert E.month_form(p, 233) == 0
    p = params_from_config(_scenario())
    p.inv1_realized_gains_tax_rate = float.fromhex("0x1.999999999999bp-4")  # one ulp above 0.1: not the same rate
    assert p.inv1_realized_gains_tax_rate != p.inv2_realized_gains_tax_rate
    assert E.month_form(p, 233) == 0


@pytest.mark.parametrize("over", [
    {"inv1_use_realized_gains_tax_system": False},                           # asset 1 untaxed on realized gains (annual rate 0)
    {"inv2_realized_gains_tax_rate": 0.0},                                   # asset 2 at a zero rate: tax mask 1
    {"inv1_realized_gains_tax_rate": 0.0, "inv2_realized_gains_tax_rate": 0.0},   # equal rates, but nothing is taxed
])
def test_one_asset_untaxed_does_not_qualify(over):
    assert E.month_form(params_from_config(_scenario(**over)), 233) == 0


def test_an_annual_gains_tax_does_not_qualify():
    # asset 1 on the annual system: its realized rate is then 0 ...
    assert E.month_form(params_from_config(_scenario(inv1_use_realized_gains_tax_system=False, inv1_annual_tax_on_gains_rate=0.2)), 233) == 0
    # ... and an annual rate on an asset that uses the realized system is not applied at all: still equal rates, no annual tax
    assert E.month_form(params_from_config(_scenario(inv1_annual_tax_on_gains_rate=0.2)), 233) == 1


def test_rates_that_need_the_exact_month_do_not_qualify():
    p = params_from_config(_scenario(inv1_realized_gains_tax_rate=1.0, inv2_realized_gains_tax_rate=1.0))
    assert E.month_form(p, 233) == 0


def test_no_contribution_growth_changes_nothing():
    assert E.month_form(params_from_config(_scenario(contribution_growth_rate_annual=0.0)), 233) == 1


def test_the_knob_forces_a_lower_mask_only():
    equal = params_from_config(_scenario())
    unequal = params_from_config(_scenario(inv2_realized_gains_tax_rate=0.15))
    for want in (0, 1):
        os.environ[KNOB] = str(want)
        assert E.month_form(equal, 233) == want
    os.environ[KNOB] = "0"
    assert E.month_form(unequal, 233) == 0
    os.environ[KNOB] = "1"
    with pytest.raises(ValueError, match=KNOB):                             # unequal rates: the bit is not available
        E.month_form(unequal, 233)
    for junk in ("2", "3", "-1", "x", "1x"):
        os.environ[KNOB] = junk
        with pytest.raises(ValueError, match=KNOB):
            E.month_form(equal, 233)


def test_shipped_scenarios_lose_their_zero_stream():
    p = params_from_config(_scenario())
    assert p.n_streams == 2                                                  # the caller's block is what it was
    assert E.kept_streams(p, 233) == [(0, -1)]                               # the indexed pension; the 0-a-month rental is gone
    assert E.kept_streams(params_from_config(_scenario("jorge.json")), 75) == [(0, -1)]


def test_lock_slots_are_numbered_over_the_kept_records():
    streams = [_stream(0.0, False), _stream(100.0, False), _stream(0.0, True), _stream(200.0, True), _stream(0.0, False),
               _stream(300.0, False), _stream(0.0, False)]
    p = params_from_config(_scenario(other_income_streams=streams))
    assert E.kept_streams(p, 233) == [(1, 0), (3, -1), (5, 1)]
    none = params_from_config(_scenario(other_income_streams=[_stream(0.0, False), _stream(0.0, True)]))
    assert E.kept_streams(none, 233) == []
    assert E.kept_streams(params_from_config(_scenario(other_income_streams=[])), 233) == []


def test_zero_records_do_not_count_against_the_inline_block():
    """20 records, every other one paying nothing: the 10 kept ones fit the by-value block of 16."""
    streams = [_stream(0.0 if i % 2 else 50.0 + i, False) for i in range(20)]
    p = params_from_config(_scenario(other_income_streams=streams))
    assert p.n_streams == 20
    assert E.kept_streams(p, 233) == [(i, i // 2) for i in range(0, 20, 2)]
