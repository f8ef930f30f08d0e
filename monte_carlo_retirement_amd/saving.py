"""Minimum-contribution search: the smallest ``monthly_contribution`` (whole cents) whose success probability reaches the
target at a fixed retirement month — the third planning question, next to `find_minimum_working_months` (when) and
`spending.search_maximum_expenses` (how much to spend).

The search is a pure function of a ``probe_levels(levels) -> [success %]`` callable, so it runs (and is tested) without a
GPU; `RetirementMonteCarloSimulator.find_minimum_monthly_contribution` plugs in the contribution fan-out probes
(`mcr_probe_contributions_rng`), which evaluate up to ``MCR_MAX_EXPENSE_FANOUT`` levels over the same random numbers.

Procedure: `search.cent_search` (bracket with a geometric ladder until a level hits, then refine), in whole cents.
``P(0) >= target`` -> ``(0.0, P(0), curve)``; a ladder that reaches the cap without a hit returns ``(-1.0, P(cap), curve)``,
with a warning.
"""

from __future__ import annotations

from typing import Callable, Optional, Sequence

from .search import SearchResult, cent_search, check, run

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
    check(levels_per_call, resolution)
    return run(cent_search(target, start, int(levels_per_call), resolution, cap, on_level, largest=False, key="monthly_contribution",
                           event="contribution_search_iter",
                           cap_warning=f"minimum-contribution search reached the cap of {cap:g} per month without reaching the target"),
               probe_levels)
