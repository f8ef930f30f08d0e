"""Required-starting-balance search: the smallest ``initial_balance`` (whole cents) whose success probability reaches the
target at a fixed retirement month — the fourth planning question, next to `find_minimum_working_months` (when),
`spending.search_maximum_expenses` (how much to spend) and `saving.search_minimum_contribution` (how much to save).  For
someone already retired (``working_months == 0``) it is the only lever, and a set of answers at several spending levels is
the safe-withdrawal-rate curve: ``12 * expenses / required balance`` at the target probability.

The search is a pure function of a ``probe_levels(levels) -> [success %]`` callable, so it runs (and is tested) without a
GPU; `RetirementMonteCarloSimulator.find_minimum_initial_balance` plugs in the scenario probes
(`mcr_probe_scenarios_rng`), which evaluate up to ``MCR_MAX_EXPENSE_FANOUT`` records over the same random numbers.

Procedure (all levels are integer cents internally) — `saving.search_minimum_contribution`'s, restated as a generator so
that several searches can run in lockstep (`spending._search` is the same device for the other direction):

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
from typing import Callable, Dict, Generator, List, Optional, Sequence

from .spending import SearchResult, _cents, _check

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


def _search(target: float, start: float, L: int, resolution: float, cap: float,
            on_level: Optional[Callable[[dict], None]], key: str = "initial_balance", event: str = "initial_balance_search_iter",
            what: str = "required-starting-balance") -> Generator[List[float], Sequence[float], SearchResult]:
    """One search: yields the levels of a call (1 .. L distinct whole-cent values), receives their probabilities, and
    returns ``(level, probability, curve)``.  ``key`` names the level in the curve and the events, ``event`` is the events'
    type and ``what`` names the search in the cap warning (`income.search_minimum_income_amount` passes its own)."""
    res_c = float(resolution) * 100.0
    cap_c = _cents(cap)
    memo: Dict[int, float] = {}
    curve: List[Dict[str, float]] = []
    state = {"call": 0, "lo": None, "hi": None}

    def evaluate(levels_c: List[int]):
        levels_c = [c for c in dict.fromkeys(levels_c) if c not in memo]
        if not levels_c:
            return
        state["call"] += 1
        probs = list((yield [c / 100.0 for c in levels_c]))
        if len(probs) != len(levels_c):
            raise RuntimeError(f"probe_levels returned {len(probs)} values for {len(levels_c)} levels")
        for c, pr in zip(levels_c, probs):
            pr = float(pr)
            memo[c] = pr
            curve.append({key: c / 100.0, "probability": pr})
            if on_level:
                on_level({"type": event, "iteration": state["call"], key: c / 100.0,
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
    yield from evaluate([0] + ladder[: L - 1])
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
            warnings.warn(f"{what} search reached the cap of {cap:g} without reaching the target",
                          RuntimeWarning, stacklevel=3)
            return -1.0, memo[cap_c], curve
        yield from evaluate(ladder[k: k + L])
    state["lo"], state["hi"] = lo, hi

    # refine
    while hi - lo > res_c:
        w = hi - lo
        n_pts = min(L, max(1, math.ceil(w / res_c) - 1), w - 1)
        step = -(-w // (n_pts + 1))     # (cents, rounded up: the largest gap is the step)
        pts = [lo + i * step for i in range(1, n_pts + 1) if lo + i * step < hi]
        if not pts:
            break
        yield from evaluate(pts)
        hits = [c for c in pts if memo[c] >= target]
        new_hi = min([hi] + hits)
        lo = max(c for c in pts + [lo] if c < new_hi)
        hi = new_hi
        state["lo"], state["hi"] = lo, hi
    return hi / 100.0, memo[hi], curve


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
    _check(levels_per_call, resolution)
    gen = _search(target, start, int(levels_per_call), resolution, cap, on_level)
    try:
        levels = next(gen)
        while True:
            levels = gen.send(probe_levels(levels))
    except StopIteration as done:
        return done.value


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
    _check(levels_per_call, resolution)
    n = len(starts)
    if monthly_expenses is not None and len(monthly_expenses) != n:
        raise ValueError(f"{len(monthly_expenses)} spending levels for {n} searches")

    def tagged(i):
        if on_level is None or monthly_expenses is None:
            return on_level
        return lambda ev: on_level(dict(ev, monthly_expenses=float(monthly_expenses[i])))

    gens = [_search(target, s, int(levels_per_call), resolution, cap, tagged(i)) for i, s in enumerate(starts)]
    results: List[Optional[SearchResult]] = [None] * n
    pending: Dict[int, List[float]] = {}
    for i, g in enumerate(gens):
        try:
            pending[i] = next(g)
        except StopIteration as done:
            results[i] = done.value
    while pending:
        rows = sorted(pending)
        probs = probe_rows(rows, [list(pending[i]) for i in rows])
        if len(probs) != len(rows):
            raise RuntimeError(f"probe_rows returned {len(probs)} rows for {len(rows)}")
        for i, row in zip(rows, probs):
            pending.pop(i)
            try:
                pending[i] = gens[i].send(list(row))
            except StopIteration as done:
                results[i] = done.value
    return results  # type: ignore[return-value]
