"""Maximum-spending search: the largest ``monthly_expenses`` (whole cents) whose success probability still reaches the
target at a fixed retirement month — the other half of the planning question `find_minimum_working_months` answers.

The search is a pure function of a ``probe_levels(levels) -> [success %]`` callable, so it runs (and is tested) without a
GPU; `RetirementMonteCarloSimulator.find_maximum_monthly_expenses` plugs in the expense fan-out probes, which evaluate up to
``MCR_MAX_EXPENSE_FANOUT`` levels at about the cost of a few.

Procedure: `search.cent_search` with ``largest`` set (bracket with a geometric ladder until a level misses, then refine), in
whole cents.  ``P(0) < target`` -> ``(-1.0, P(0), curve)``; a ladder that reaches the cap without a miss returns the cap, with a
warning.  `search_maximum_expenses_many` runs one search per working month in lockstep (`search.run_many`): each round, every
unfinished search's levels go into ONE rectangular ``probe_rows`` call (the grid probe, `mcr_probe_grid_rng`).
"""

from __future__ import annotations

from typing import Callable, List, Optional, Sequence

from .search import SearchResult, cent_search, check, run, run_many

EXPENSE_CAP = 1e9   # per month


def _steps(target, start, levels_per_call, resolution, cap, on_level):
    return cent_search(target, start, int(levels_per_call), resolution, cap, on_level, largest=True, key="monthly_expenses",
                       event="expense_search_iter",
                       cap_warning=f"maximum-spending search reached the cap of {cap:g} per month without missing the target")


def search_maximum_expenses(
    probe_levels: Callable[[Sequence[float]], Sequence[float]],
    target: float,
    start: float,
    levels_per_call: int = 15,
    resolution: float = 1.0,
    cap: float = EXPENSE_CAP,
    on_level: Optional[Callable[[dict], None]] = None,
) -> SearchResult:
    """Returns ``(expenses, probability, curve)``: the largest level found with ``P >= target`` (``-1.0`` when even zero
    spending misses), its probability, and ``{"monthly_expenses", "probability"}`` per evaluated level in evaluation order.
    ``on_level`` receives one ``"expense_search_iter"`` event per evaluated level."""
    check(levels_per_call, resolution)
    return run(_steps(target, start, levels_per_call, resolution, cap, on_level), probe_levels)


def search_maximum_expenses_many(
    probe_rows: Callable[[List[int], List[List[float]]], Sequence[Sequence[float]]],
    target: float,
    starts: Sequence[float],
    levels_per_call: int = 15,
    resolution: float = 1.0,
    cap: float = EXPENSE_CAP,
    on_level: Optional[Callable[[dict], None]] = None,
    working_months: Optional[Sequence[int]] = None,
) -> List[SearchResult]:
    """One `search_maximum_expenses` per entry of ``starts``, run in lockstep.  Each round calls ``probe_rows(rows,
    levels_2d) -> [len(rows)][width]`` once: ``rows`` are the indices of the unfinished searches, ``levels_2d`` their next
    levels, each row padded to the widest by repeating its own last level (padded results are discarded).  Search ``i``
    returns exactly what ``search_maximum_expenses`` would with ``start = starts[i]`` and probabilities from row ``i``; its
    ``on_level`` events also carry ``"working_months": working_months[i]`` (``i`` when not given)."""
    check(levels_per_call, resolution)
    n = len(starts)
    keys = list(range(n)) if working_months is None else [int(m) for m in working_months]
    if len(keys) != n:
        raise ValueError(f"{len(keys)} working months for {n} searches")
    return run_many(lambda i, on_i: _steps(target, starts[i], levels_per_call, resolution, cap, on_i), n, probe_rows, pad=True,
                    on_level=on_level, tag=lambda i: {"working_months": keys[i]})
