"""The default form of a screened launch's re-run depends on the expected list (csrc/mcr_hip.hip, rerun_producers_of: the
64-path form up to 80 000 expected paths, the 256-path form beyond).  That choice is made inside the launch and moves no
answer a caller can ask for without a device: which launches take the screened route, and what the knob accepts, are what
they were."""

from __future__ import annotations

import json
import os

import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

WM = 233
KNOBS = ("MCR_K1_SCREEN", "MCR_K1_SCREEN_MIN_PATHS", "MCR_K1_SCREEN_EXPECTED", "MCR_K1_RERUN_PRODUCERS", "MCR_K1_SPLIT_MAX_WAVES",
         "MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS", "MCR_K1_SEGMENT_ORDER", "MCR_K1_GROWTH_FORM",
         "MCR_K1_MONTH_FORM", "MCR_K1_STREAM_FORM")


@pytest.fixture()
def params(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        return params_from_config(Config(**json.load(fh)))


def test_the_route_of_300_and_of_a_million_paths_is_what_it_was(params):
    assert not E.screen(params, WM, 300)
    assert E.screen(params, WM, 10**6)


@pytest.mark.parametrize("forced", ["1", "2"])
def test_forcing_a_form_moves_no_route(params, monkeypatch, forced):
    monkeypatch.setenv("MCR_K1_RERUN_PRODUCERS", forced)
    assert not E.screen(params, WM, 300)
    assert E.screen(params, WM, 10**6)


@pytest.mark.parametrize("junk", ["0", "3", "two", "2 ", "12"])
def test_junk_in_the_knob_still_raises(params, monkeypatch, junk):
    monkeypatch.setenv("MCR_K1_RERUN_PRODUCERS", junk)
    for n in (300, 10**6):
        with pytest.raises(ValueError, match="MCR_K1_RERUN_PRODUCERS"):
            E.screen(params, WM, n)
