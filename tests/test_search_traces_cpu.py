"""The seven public level searches, replayed on fixed stub curves and held to traces recorded before the searches were folded
onto one core (`tests/golden/search_traces.json` names the commit): the probe-call sequence, the returned tuples, every event
with its key order, and every warning's text.  Each warning must also be attributed to the caller of the public function,
which here is this file.

    python tests/test_search_traces_cpu.py --record COMMIT      (rewrites the fixture from the modules as they are)
"""

from __future__ import annotations

import json
import os
import sys
import warnings

import pytest

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from monte_carlo_retirement_amd.income import search_minimum_income_amount
from monte_carlo_retirement_amd.nestegg import search_minimum_initial_balance, search_minimum_initial_balance_many
from monte_carlo_retirement_amd.saving import search_minimum_contribution
from monte_carlo_retirement_amd.spending import search_maximum_expenses, search_maximum_expenses_many
from monte_carlo_retirement_amd.stress import search_breakeven

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_traces.json")
THIS_FILE = os.path.abspath(__file__)
TARGET = 90.0


# ---- stub curves: success % as a function of the level, rising (a minimum search) or falling (the maximum search) ----------
def _noise(x: float, scale: float) -> float:
    """A fixed pseudo-random value in [-0.5, 0.5) per level (levels are multiples of ``scale``)."""
    return ((int(round(x / scale)) * 2654435761 + 12345) % 1000) / 1000.0 - 0.5


def curve(kind: str, at: float = 0.0, rising: bool = True, width: float = 1.0, scale: float = 0.01):
    """``step``: 99 % on the good side of ``at`` (``at`` included), 10 % on the other.  ``noisy``: a ramp through the target at
    ``at``, ``width`` wide, with up to +-6 points of per-level noise, so that hits and misses interleave near ``at``.
    ``always`` / ``never``: 100 % / 0 % everywhere."""
    side = 1.0 if rising else -1.0

    def p(x: float) -> float:
        if kind == "always":
            return 100.0
        if kind == "never":
            return 0.0
        d = side * (x - at)
        if kind == "step":
            return 99.0 if d >= 0 else 10.0
        return min(100.0, max(0.0, TARGET + 8.0 * d / width + 12.0 * _noise(x, scale)))

    return p


def _single(fn, rising, kind, at, L, res, cap=None, start=1000.0, width=50.0):
    def run(calls, events):
        p = curve(kind, at, rising, width)

        def probe(levels):
            calls.append(list(levels))
            return [p(x) for x in levels]

        kw = {} if cap is None else {"cap": cap}
        return fn(probe, TARGET, start, levels_per_call=L, resolution=res, on_level=events.append, **kw)
    return run


def _many(fn, rising, specs, L, res, cap=None, **tags):
    """``specs``: ``(kind, at, start)`` per search; the probe answers a padded row with one value per level it was given."""
    def run(calls, events):
        ps = [curve(kind, at, rising, 2.0) for kind, at, _ in specs]

        def probe_rows(rows, levels_2d):
            calls.append([list(rows), [list(r) for r in levels_2d]])
            return [[ps[i](x) for x in row] for i, row in zip(rows, levels_2d)]

        kw = dict(tags, **({} if cap is None else {"cap": cap}))
        return fn(probe_rows, TARGET, [s for _, _, s in specs], levels_per_call=L, resolution=res, on_level=events.append, **kw)
    return run


def _breakeven(field, base, kind, at, rising, L, res=1e-4, window=0.25, width=0.01):
    def run(calls, events):
        p = curve(kind, at, rising, width, scale=res)

        def probe(levels):
            calls.append(list(levels))
            return [p(x) for x in levels]

        return search_breakeven(probe, TARGET, field, base, window=window, resolution=res, levels_per_call=L, on_level=events.append)
    return run


def _cases():
    cases = {}
    singles = (("expenses", search_maximum_expenses, False), ("contribution", search_minimum_contribution, True),
               ("initial_balance", search_minimum_initial_balance, True), ("income_amount", search_minimum_income_amount, True))
    for name, fn, rising in singles:
        cases[f"{name}-step-L15-res1"] = _single(fn, rising, "step", 43.21, 15, 1.0, start=10.0)
        cases[f"{name}-step-L1-res0.5"] = _single(fn, rising, "step", 777.77, 1, 0.5, start=100.0)
        cases[f"{name}-step-L2-res0.01"] = _single(fn, rising, "step", 12.34, 2, 0.01, start=10.0)
        cases[f"{name}-noisy-L8-res0.5"] = _single(fn, rising, "noisy", 25.0, 8, 0.5, start=10.0, width=1.0)
        cases[f"{name}-noisy-L15-res0.1"] = _single(fn, rising, "noisy", 6.1, 15, 0.1, start=1.0, width=0.2)
        cases[f"{name}-noisy-L2-res1"] = _single(fn, rising, "noisy", 15.0, 2, 1.0, start=0.0, width=3.0)
        cases[f"{name}-always-L8"] = _single(fn, rising, "always", 0.0, 8, 1.0)
        cases[f"{name}-always-L2-cap5000"] = _single(fn, rising, "always", 0.0, 2, 0.5, cap=5000.0)
        cases[f"{name}-never-L8-cap5000"] = _single(fn, rising, "never", 0.0, 8, 1.0, cap=5000.0)
        cases[f"{name}-never-L1-cap5000"] = _single(fn, rising, "never", 0.0, 1, 0.01, cap=5000.0, start=3000.0)
    specs = (("step", 23.45, 10.0), ("never", 0.0, 10.0), ("noisy", 9.0, 40.0), ("step", 1500.0, 100.0), ("always", 0.0, 5.0))
    for name, fn, rising, tags in (("expenses_many", search_maximum_expenses_many, False, {"working_months": [12, 120, 240, 360, 480]}),
                                   ("initial_balance_many", search_minimum_initial_balance_many, True,
                                    {"monthly_expenses": [1000.0, 2000.0, 3000.5, 4000.0, 5000.0]})):
        cases[f"{name}-L8-res1-tagged"] = _many(fn, rising, specs, 8, 1.0, cap=2000.0, **tags)
        cases[f"{name}-L15-res2"] = _many(fn, rising, specs[:3], 15, 2.0, cap=4000.0)
        cases[f"{name}-L1-res1"] = _many(fn, rising, specs[:3], 1, 1.0, cap=5000.0)
        cases[f"{name}-L2-res0.01"] = _many(fn, rising, (specs[0], specs[2]), 2, 0.01, cap=5000.0)
    # break-even: success rises with a mean of returns and falls with a volatility or with inflation
    cases["breakeven-equity_mean-step-L15"] = _breakeven("inv1_returns_mean", 0.07, "step", 0.0312, True, 15, window=0.1)
    cases["breakeven-equity_mean-noisy-L8"] = _breakeven("inv1_returns_mean", 0.07, "noisy", 0.0155, True, 8, window=0.1, width=0.002)
    cases["breakeven-equity_mean-step-L3"] = _breakeven("inv1_returns_mean", 0.07, "step", -0.0501, True, 3)
    cases["breakeven-inflation_mean-step-L8"] = _breakeven("inflation_rate_mean", 0.03, "step", 0.0777, False, 8, window=0.06)
    cases["breakeven-equity_vol-noisy-L4-clipped"] = _breakeven("inv1_returns_volatility", 0.15, "noisy", 0.31, False, 4, width=0.004)
    cases["breakeven-equity_vol-step-res1e-3"] = _breakeven("inv1_returns_volatility", 0.15, "step", 0.2, False, 8, res=1e-3)
    cases["breakeven-premium_mean-holds_at_window_end"] = _breakeven("inv2_premium_over_inflation_mean", 0.01, "always", 0.0, True, 8)
    cases["breakeven-inflation_vol-holds_at_clipped_end"] = _breakeven("inflation_rate_volatility", 0.01, "step", 0.3, False, 5, window=0.05)
    cases["breakeven-equity_mean-not_reached"] = _breakeven("inv1_returns_mean", 0.07, "never", 0.0, True, 8)
    cases["breakeven-equity_vol-not_reached-clipped"] = _breakeven("inv1_returns_volatility", 0.15, "never", 0.0, False, 3, window=0.5)
    cases["breakeven-equity_mean-narrow-window"] = _breakeven("inv1_returns_mean", 0.07, "step", 0.0699, True, 15, window=0.0003)
    return cases


CASES = _cases()


def trace(run):
    """One case's record, in JSON's own types.  Events become lists of ``[key, value]`` pairs so that key order is held."""
    calls, events = [], []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        result = run(calls, events)
    doc = {"calls": calls, "result": result, "events": [[[k, v] for k, v in ev.items()] for ev in events],
           "warnings": [str(w.message) for w in caught]}
    return json.loads(json.dumps(doc)), [(w.category, os.path.abspath(w.filename)) for w in caught]


if __name__ != "__main__":
    with open(FIXTURE) as _fh:
        GOLDEN = json.load(_fh)


def test_fixture_covers_exactly_these_cases():
    assert sorted(GOLDEN["cases"]) == sorted(CASES)
    kinds = {"found": 0, "holds_at_window_end": 0, "not_reached": 0}
    for name, doc in GOLDEN["cases"].items():
        if name.startswith("breakeven"):
            kinds[doc["result"][3]] += 1
    assert all(kinds.values()), kinds
    assert sum(1 for d in GOLDEN["cases"].values() if d["warnings"]) >= 12      # the cap and the not-reached routes are in the set


@pytest.mark.parametrize("name", sorted(CASES))
def test_search_replays_the_recorded_trace(name):
    got, attributed = trace(CASES[name])
    want = GOLDEN["cases"][name]
    assert got["calls"] == want["calls"]
    assert got["result"] == want["result"]
    assert got["events"] == want["events"]
    assert got["warnings"] == want["warnings"]
    assert attributed == [(RuntimeWarning, THIS_FILE)] * len(want["warnings"])


def test_many_searches_finish_in_different_rounds():
    for name in ("expenses_many-L8-res1-tagged", "initial_balance_many-L8-res1-tagged"):
        rows = [tuple(c[0]) for c in GOLDEN["cases"][name]["calls"]]
        assert len(set(rows)) >= 3 and rows[0] == (0, 1, 2, 3, 4), rows


if __name__ == "__main__":
    assert sys.argv[1] == "--record" and len(sys.argv) == 3, __doc__
    doc = {"recorded_from_commit": sys.argv[2], "target": TARGET, "cases": {name: trace(run)[0] for name, run in sorted(CASES.items())}}
    with open(FIXTURE, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    levels = sum(len(c["events"]) for c in doc["cases"].values())
    print(f"{len(doc['cases'])} cases, {levels} evaluated levels, {os.path.getsize(FIXTURE)} bytes -> {FIXTURE}")
