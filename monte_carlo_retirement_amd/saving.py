"""Minimum-contribution search: the smallest ``monthly_contribution`` (whole cents) whose success probability reaches the
target at a fixed retirement month — the third planning question, next to `find_minimum_working_months` (when) and
`spending.search_maximum_expenses` (how much to spend).

The search is a pure function of a ``probe_levels(levels) -> [success %]`` callable, so it runs (and is tested) without a
GPU; `RetirementMonteCarloSimulator.find_minimum_monthly_contribution` plugs in the contribution fan-out probes
(`mcr_probe_contributions_rng`), which evaluate up to ``MCR_MAX_EXPENSE_FANOUT`` levels over the same random numbers.

Procedure (all levels are integer cents internally) — `spending`'s search with the direction flipped:

* ``P(0)`` is evaluated with the first rungs of the bracket; ``P(0) >= target`` -> ``(0.0, P(0), curve)``.
* BRACKET: a geometric ladder ``start * 2**k`` (``levels_per_call`` levels a call, capped at ``cap``) until a level hits.
  ``hi`` = the first hit, ``lo`` = the last miss below it.  A ladder that reaches the cap without a hit returns
  ``(-1.0, P(cap), curve)``, with a warning.
* REFINE: up to ``levels_per_call`` evenly spaced interior points of ``(lo, hi)`` (never more than it takes to get the gaps
  down to ``resolution``), spaced by the cent-rounded-up step.  New ``hi`` = the smallest hit among the points and ``hi``,
  new ``lo`` = the largest evaluated level below it.  Monte Carlo estimates are not monotone in the level, but this keeps
  ``P(hi) >= target > P(lo)`` with ``lo`` and ``hi`` adjacent among the levels evaluated in ``(lo, hi)``.  Stops when
  ``hi - lo <= resolution``: ``ceil(log_{L+1}(range / resolution))`` calls for a resolution of whole cents.
"""

from __future__ import annotations

import math
import warnings
from typing import Callable, Dict, List, Optional, Sequence

from .spending import SearchResult, _cents, _check

#: Highest contribution the search tries, per month.  The engine's division is bit-identical to ``a / b`` while balances
#: live in 1e-6 .. 1e15 (mcr_math.h, fdiv): 1e8 a month is 1.2e9 a year and 8.4e10 over the working-month search's 70-year
#: horizon, which leaves four orders of magnitude for market growth before balances approach 1e15.  A target that 1e8 a
#: month does not reach is not reached by saving more.
CONTRIBUTION_CAP = 1e8


def search_minimum_contribution(
    probe_levels: Callable[[Sequence[float]], Sequence[float]],
    target: float,
    start: float,
    levels_per_call: int = 15,
    resolution: float = 1.0,
    cap: float = CONTRIBUTION_CAP,
    on_level: Optional[Callable[[dict], None]] = None,
) -> SearchResult:
    """Returns ``(contribution, probability, curve)``: the smallest level found with ``P >= target`` (``0.0`` when no
    contribution is needed, ``-1.0`` when even ``cap`` misses), its probability, and ``{"monthly_contribution",
    "probability"}`` per evaluated level in evaluation order.  ``on_level`` receives one ``"contribution_search_iter"``
    event per evaluated level."""
    _check(levels_per_call, resolution)
    L = int(levels_per_call)
    res_c = float(resolution) * 100.0
    cap_c = _cents(cap)
    memo: Dict[int, float] = {}
    curve: List[Dict[str, float]] = []
    state = {"call": 0, "lo": None, "hi": None}

    def evaluate(levels_c: List[int]) -> None:
        levels_c = [c for c in dict.fromkeys(levels_c) if c not in memo]
        if not levels_c:
            return
        state["call"] += 1
        probs = list(probe_levels([c / 100.0 for c in levels_c]))
        if len(probs) != len(levels_c):
            raise RuntimeError(f"probe_levels returned {len(probs)} values for {len(levels_c)} levels")
        for c, pr in zip(levels_c, probs):
            pr = float(pr)
            memo[c] = pr
            curve.append({"monthly_contribution": c / 100.0, "probability": pr})
            if on_level:
                on_level({"type": "contribution_search_iter", "iteration": state["call"], "monthly_contribution": c / 100.0,
                          "probability": round(pr, 2), "target": target,
                          "lo": None if state["lo"] is None else state["lo"] / 100.0,
                          "hi": None if state["hi"] is None else state["hi"] / 100.0})

    # bracket: 0 and the first rungs in one call, then L rungs a call
    rung = max(_cents(max(float(start), 1.0)), 1)
    ladder: List[int] = []
    while True:
        ladder.append(min(rung, cap_c))
        if rung >= cap_c:
            break
        rung *= 2
    evaluate([0] + ladder[: L - 1])
    if memo[0] >= target:
        return 0.0, memo[0], curve
    lo, hi = 0, None
    while hi is None:
        for c in ladder:
            if c not in memo:
                break
            if memo[c] >= target:
                hi = c
                break
            lo = c
        if hi is not None:
            break
        k = next((i for i, c in enumerate(ladder) if c not in memo), None)
        if k is None:   # every rung up to the cap missed
            warnings.warn(f"minimum-contribution search reached the cap of {cap:g} per month without reaching the target",
                          RuntimeWarning, stacklevel=2)
            return -1.0, memo[cap_c], curve
        evaluate(ladder[k: k + L])
    state["lo"], state["hi"] = lo, hi

    # refine
    while hi - lo > res_c:
        w = hi - lo
        n_pts = min(L, max(1, math.ceil(w / res_c) - 1), w - 1)
        step = -(-w // (n_pts + 1))     # (cents, rounded up: the largest gap is the step)
        pts = [lo + i * step for i in range(1, n_pts + 1) if lo + i * step < hi]
        if not pts:
            break
        evaluate(pts)
        hits = [c for c in pts if memo[c] >= target]
        new_hi = min([hi] + hits)
        lo = max(c for c in pts + [lo] if c < new_hi)
        hi = new_hi
        state["lo"], state["hi"] = lo, hi
    return hi / 100.0, memo[hi], curve
