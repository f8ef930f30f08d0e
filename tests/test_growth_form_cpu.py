"""The host's choice of a launch's GROWTH FORM (csrc/mcr_hip.hip: growth_form_of; DESIGN.md "growth forms"), through
mcr_k1_growth_form — no device needed.

The documented bound: a launch takes the narrow exp window when, for each of its three monthly log-return series
x = a + b z (a = mu_log / 12, b = sigma_log / sqrt 12),

    (|a| + c |b| Zmax) 512 / ln 2 <= 255 - 1,     Zmax = sqrt(-2 ln 2^-33),  c = 1 (equity, premium), |rho| + sqrt(1 - rho^2) (inflation)

and drops the rho term of the inflation series when rho = 0.  The boundary volatilities below are solved from THAT statement."""

from __future__ import annotations

import json
import math
import os

import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

KNOB = "MCR_K1_GROWTH_FORM"
ZMAX = math.sqrt(-2.0 * math.log(2.0 ** -33))
XMAX = (255 - 1) * math.log(2.0) / 512.0


@pytest.fixture(autouse=True)
def _no_knob():
    old = os.environ.pop(KNOB, None)
    yield
    os.environ.pop(KNOB, None)
    if old is not None:
        os.environ[KNOB] = old


def _config(**over):
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        return Config(**dict(json.load(fh), **over))


def _s60():
    return _config(initial_balance=2.0e6, inv1_returns_volatility=0.15, equity_inflation_correlation=0.3, seed=12345)


def _boundary_sigma_log(mu_log, c=1.0):
    """sigma_log at which (|a| + c b Zmax) 512 / ln 2 = 254 exactly."""
    return (XMAX - abs(mu_log) / 12.0) * math.sqrt(12.0) / (c * ZMAX)


def test_zmax_is_the_generators_own_bound():
    assert ZMAX == pytest.approx(6.764, abs=1e-3)


def test_shipped_scenarios():
    assert E.growth_form(params_from_config(_config()), 233) == 3          # config.json: 2 % volatilities, rho = 0
    assert E.growth_form(params_from_config(_s60()), 120) == 1             # S60: 15 % volatility qualifies, rho = 0.3 does not


@pytest.mark.parametrize("series", ["inv1", "inf", "prem"])
@pytest.mark.parametrize("rho", [0.0, 0.3])
def test_volatility_just_below_and_just_above_the_bound(series, rho):
    p = params_from_config(_s60())
    p.equity_inflation_rho = rho
    c = abs(rho) + math.sqrt(1.0 - rho * rho) if series == "inf" else 1.0
    s = _boundary_sigma_log(getattr(p, f"{series}_mu_log"), c)
    assert 0.1 < s < 0.2                                                    # (annual log-volatility of ~16 %: a plausible scenario)
    setattr(p, f"{series}_sigma_log", s * (1.0 - 1e-9))
    assert E.growth_form(p, 120) == (3 if rho == 0.0 else 1)
    setattr(p, f"{series}_sigma_log", s * (1.0 + 1e-9))
    assert E.growth_form(p, 120) == 0


def test_the_knob_forces_a_lower_mask_only():
    config, s60 = params_from_config(_config()), params_from_config(_s60())
    wide = params_from_config(_s60())
    wide.inv1_sigma_log = _boundary_sigma_log(wide.inv1_mu_log) * 1.01
    for want in (0, 1, 3):
        os.environ[KNOB] = str(want)
        assert E.growth_form(config, 233) == want
    for want in (0, 1):
        os.environ[KNOB] = str(want)
        assert E.growth_form(s60, 120) == want
    os.environ[KNOB] = "3"
    with pytest.raises(ValueError, match=KNOB):                             # rho = 0.3: bit 1 is not available
        E.growth_form(s60, 120)
    for want in (1, 3):
        os.environ[KNOB] = str(want)
        with pytest.raises(ValueError, match=KNOB):                         # outside the window: no bit is
            E.growth_form(wide, 120)
    os.environ[KNOB] = "0"
    assert E.growth_form(wide, 120) == 0
    for junk in ("2", "4", "-1", "x", "1x"):                                # (mask 2, rho = 0 alone, is not built)
        os.environ[KNOB] = junk
        with pytest.raises(ValueError, match=KNOB):
            E.growth_form(config, 233)
