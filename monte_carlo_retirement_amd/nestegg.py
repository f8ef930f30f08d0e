"""Required-starting-balance search: the smallest ``initial_balance`` (whole cents) whose success probability reaches the
target at a fixed retirement month — the fourth planning question, next to `find_minimum_working_months` (when),
`spending.search_maximum_expenses` (how much to spend) and `saving.search_minimum_contribution` (how much to save).  For
someone already retired (``working_months == 0``) it is the only lever, and a set of answers at several spending levels is
the safe-withdrawal-rate curve: ``12 * expenses / required balance`` at the target probability.

The search is a pure function of a ``probe_levels(levels) -> [success %]`` callable, so it runs (and is tested) without a
GPU; `RetirementMonteCarloSimulator.find_minimum_initial_balance` plugs in the scenario probes
(`mcr_probe_scenarios_rng`), which evaluate up to ``MCR_MAX_EXPENSE_FANOUT`` records over the same random numbers.

Procedure: `search.cent_search` (bracket with a geometric ladder until a level hits, then refine), in whole cents.
``P(0) >= target`` -> ``(0.0, P(0), curve)``; a ladder that reaches the cap without a hit returns ``(-1.0, P(cap), curve)``,
with a warning.  `search_minimum_initial_balance_many` runs several searches in lockstep (`search.run_many`).
"""

from __future__ import annotations

from typing import Callable, List, Optional, Sequence

from .search import SearchResult, Steps, cent_search, check, run, run_many

#: Highest starting balance the search tries.  The engine's division is bit-identical to ``a / b`` while balances live in
#: 1e-6 .. 1e15 (mcr_math.h, fdiv): a start of 1e11 leaves four orders of magnitude for market growth and contributions
#: before a balance approaches 1e15 — the headroom `saving.CONTRIBUTION_CAP` keeps (1e8 a month adds up to 8.4e10 over the
#: working-month search's 70-year horizon, the same order as this cap).  A target that 1e11 up front does not reach is not
#: reached by starting with more.
INITIAL_BALANCE_CAP = 1e11

#: the keys `RetirementMonteCarloSimulator.success_probability_by_scenarios` takes in a scenario mapping, in record order
SCENARIO_FIELDS = ("initial_balance", "monthly_contribution", "monthly_expenses")


def scenario_records(scenarios: Sequence[dict], defaults: Sequence[float]) -> List[tuple]:
    """``(initial_balance, monthly_contribution, monthly_expenses)`` per mapping of ``scenarios``: a missing key takes its
    entry of ``defaults`` (the config's three values, in `SCENARIO_FIELDS` order), an unknown key raises ``ValueError``."""
    records = []
    for k, s in enumerate(scenarios):
        unknown = sorted(set(s) - set(SCENARIO_FIELDS))
        if unknown:
            raise ValueError(f"scenarios[{k}]: unknown key(s) {unknown}; a scenario may set {list(SCENARIO_FIELDS)}")
        records.append(tuple(float(s.get(f, d)) for f, d in zip(SCENARIO_FIELDS, defaults)))
    return records


def _steps(target: float, start: float, levels_per_call: int, resolution: float, cap: float,
           on_level: Optional[Callable[[dict], None]], key: str = "initial_balance", event: str = "initial_balance_search_iter",
           what: str = "required-starting-balance") -> Steps:
    """The search's generator.  ``key`` names the level in the curve and the events, ``event`` is the events' type and ``what``
    names the search in the cap warning (`income.search_minimum_income_amount` passes its own)."""
    return cent_search(target, start, int(levels_per_call), resolution, cap, on_level, largest=False, key=key, event=event,
                       cap_warning=f"{what} search reached the cap of {cap:g} without reaching the target")


def search_minimum_initial_balance(
    probe_levels: Callable[[Sequence[float]], Sequence[float]],
    target: float,
    start: float,
    levels_per_call: int = 15,
    resolution: float = 1.0,
    cap: float = INITIAL_BALANCE_CAP,
    on_level: Optional[Callable[[dict], None]] = None,
) -> SearchResult:
    """Returns ``(initial_balance, probability, curve)``: the smallest level found with ``P >= target`` (``0.0`` when no
    starting balance is needed, ``-1.0`` when even ``cap`` misses), its probability, and ``{"initial_balance",
    "probability"}`` per evaluated level in evaluation order.  ``on_level`` receives one ``"initial_balance_search_iter"``
    event per evaluated level."""
    check(levels_per_call, resolution)
    return run(_steps(target, start, levels_per_call, resolution, cap, on_level), probe_levels)


def search_minimum_initial_balance_many(
    probe_rows: Callable[[List[int], List[List[float]]], Sequence[Sequence[float]]],
    target: float,
    starts: Sequence[float],
    levels_per_call: int = 15,
    resolution: float = 1.0,
    cap: float = INITIAL_BALANCE_CAP,
    on_level: Optional[Callable[[dict], None]] = None,
    monthly_expenses: Optional[Sequence[float]] = None,
) -> List[SearchResult]:
    """One `search_minimum_initial_balance` per entry of ``starts``, run in lockstep.  Each round calls ``probe_rows(rows,
    levels_2d) -> [len(rows)][len(levels_2d[r])]`` once: ``rows`` are the indices of the unfinished searches, ``levels_2d``
    their next levels (rows may differ in length: a scenario probe takes any list of points, nothing is padded).  Search
    ``i`` returns exactly what ``search_minimum_initial_balance`` would with ``start = starts[i]`` and probabilities from
    row ``i``; with ``monthly_expenses`` given (one per search: the withdrawal-rate curve) its ``on_level`` events also
    carry ``"monthly_expenses": monthly_expenses[i]``."""
    check(levels_per_call, resolution)
    n = len(starts)
    if monthly_expenses is not None and len(monthly_expenses) != n:
        raise ValueError(f"{len(monthly_expenses)} spending levels for {n} searches")
    tag = None if monthly_expenses is None else (lambda i: {"monthly_expenses": float(monthly_expenses[i])})
    return run_many(lambda i, on_i: _steps(target, starts[i], levels_per_call, resolution, cap, on_i), n, probe_rows, pad=False,
                    on_level=on_level, tag=tag)
