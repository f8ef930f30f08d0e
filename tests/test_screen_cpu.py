"""The host's choice of the SCREENED route of a count-only launch (csrc/mcr_hip.hip: screen_route_of; DESIGN.md "screened
count-only launches"), through mcr_k1_screen — no device needed.

A launch is screened when its parameters qualify (no annual-gains tax, the tolerance month, at most two paying income records,
all inflation-indexed), it runs on the engine's own stream without the in-kernel histogram, and it has at least
MCR_K1_SCREEN_MIN_PATHS paths.  MCR_K1_SCREEN=0 turns the route off, =1 takes it at any size, and any knob that addresses the
classic kernels sends the launch there."""

from __future__ import annotations

import json
import os
import re

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E

SCREEN_KNOBS = ("MCR_K1_SCREEN", "MCR_K1_SCREEN_MIN_PATHS", "MCR_K1_SCREEN_EXPECTED")
CLASSIC_KNOBS = {"MCR_K1_SEGMENTS": "0", "MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENT_ORDER": "0,1", "MCR_K1_SEGMENT_POLLS": "1",
                 "MCR_K1_GROWTH_FORM": "0", "MCR_K1_MONTH_FORM": "0", "MCR_K1_STREAM_FORM": "0"}
DEFAULT_PATHS = 1_000_000      # the shipped default size of a final run


@pytest.fixture(autouse=True)
def _no_knobs():
    names = SCREEN_KNOBS + tuple(CLASSIC_KNOBS)
    old = {k: os.environ.pop(k, None) for k in names}
    yield
    for k in names:
        os.environ.pop(k, None)
        if old[k] is not None:
            os.environ[k] = old[k]


def _scenario(name="config.json", **over):
    with open(os.path.join(REPO, "scenarios", name)) as fh:
        return Config(**dict(json.load(fh), **over))


def _stream(amount, indexed=True, start=62.0, years=None):
    return {"name": f"s{amount}", "monthly_amount_today": amount, "start_at_age": start, "duration_years": years,
            "inflation_indexed": indexed, "tax_rate": 0.2}


def _screened(cfg, wm=233, n=DEFAULT_PATHS, **kw):
    return E.screen(params_from_config(cfg), wm, n, **kw)


def test_the_shipped_scenarios_qualify_at_the_default_size():
    assert _screened(_scenario())
    assert _screened(_scenario("jorge.json"), wm=75)


def test_small_launches_take_the_classic_route_unless_forced():
    assert not _screened(_scenario(), n=300)
    assert not _screened(_scenario(), n=0)
    os.environ["MCR_K1_SCREEN"] = "1"
    assert _screened(_scenario(), n=300)
    assert not _screened(_scenario(), n=2**32)          # the list holds 32-bit local indices
    os.environ["MCR_K1_SCREEN"] = "0"
    assert not _screened(_scenario())


def test_the_minimum_size_knob_moves_the_threshold():
    os.environ["MCR_K1_SCREEN_MIN_PATHS"] = "1000"
    assert _screened(_scenario(), n=1000) and not _screened(_scenario(), n=999)
    os.environ["MCR_K1_SCREEN_MIN_PATHS"] = "4000000"
    assert not _screened(_scenario())


def test_plans_the_screening_month_does_not_cover_do_not_qualify():
    assert not _screened(_scenario(inv1_use_realized_gains_tax_system=False, inv1_annual_tax_on_gains_rate=0.2))
    assert not _screened(_scenario(other_income_streams=[_stream(800.0), _stream(300.0), _stream(100.0)]))
    assert not _screened(_scenario(other_income_streams=[_stream(800.0), _stream(50.0, indexed=False)]))
    assert not _screened(_scenario(inv1_realized_gains_tax_rate=1.0, inv2_realized_gains_tax_rate=1.0))    # the exact month
    assert _screened(_scenario(other_income_streams=[_stream(800.0), _stream(300.0, start=70.0)]))
    assert _screened(_scenario(other_income_streams=[_stream(800.0), _stream(0.0, indexed=False), _stream(300.0)]))   # a record that pays nothing is dropped
    assert _screened(_scenario(other_income_streams=[]))


def test_the_histogram_and_the_other_streams_do_not_qualify():
    cfg = _scenario()
    assert not _screened(cfg, hist_n_bins=64)
    assert not _screened(cfg, rng=N.numpy_rng(12345, 0))
    table = np.random.default_rng(1).standard_normal((120, 3))
    for scheme in (N.MCR_HISTORY_BLOCK, N.MCR_HISTORY_STATIONARY):
        assert not _screened(cfg, rng=N.history_rng(7, table, 12, scheme))
    assert _screened(cfg, rng=N.philox_rng(12345))


@pytest.mark.parametrize("knob", sorted(CLASSIC_KNOBS))
def test_any_knob_of_the_classic_kernels_gives_the_classic_route(knob):
    os.environ[knob] = CLASSIC_KNOBS[knob]
    assert not _screened(_scenario())
    os.environ["MCR_K1_SCREEN"] = "1"                    # ... also when the route is forced
    assert not _screened(_scenario())


def test_junk_in_the_knobs_is_an_error():
    for junk in ("2", "-1", "yes", "1x"):
        os.environ["MCR_K1_SCREEN"] = junk
        with pytest.raises(ValueError, match="MCR_K1_SCREEN"):
            _screened(_scenario())
    os.environ["MCR_K1_SCREEN"] = "1"
    os.environ["MCR_K1_SCREEN_MIN_PATHS"] = "many"
    with pytest.raises(ValueError, match="MCR_K1_SCREEN_MIN_PATHS"):
        _screened(_scenario())


def test_header_and_binding_agree():
    hdr = open(os.path.join(REPO, "include", "mcr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mcr_[a-z0-9_]+)\s*\(", hdr))
    lib = N.load_library()
    for sym in ("mcr_k1_screen", "mcr_screen_paths_rng"):
        assert sym in declared and sym in N.ABI_SYMBOLS and hasattr(lib, sym), sym
    assert declared == set(N.ABI_SYMBOLS)
    assert lib.mcr_abi_version() == N.MCR_ABI_VERSION == 8
    assert re.search(r"#define\s+MCR_SCREEN_SAFE\s+0\b", hdr) and re.search(r"#define\s+MCR_SCREEN_DOUBTFUL\s+1\b", hdr)
