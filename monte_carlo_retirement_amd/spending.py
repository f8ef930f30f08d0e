"""Maximum-spending search: the largest ``monthly_expenses`` (whole cents) whose success probability still reaches the
target at a fixed retirement month — the other half of the planning question `find_minimum_working_months` answers.

The search is a pure function of a ``probe_levels(levels) -> [success %]`` callable, so it runs (and is tested) without a
GPU; `RetirementMonteCarloSimulator.find_maximum_monthly_expenses` plugs in the expense fan-out probes, which evaluate up to
``MCR_MAX_EXPENSE_FANOUT`` levels at about the cost of a few.

Procedure (all levels are integer cents internally):

* ``P(0)`` is evaluated with the first rung of the bracket; ``P(0) < target`` -> ``(-1.0, P(0), curve)``.
* BRACKET: a geometric ladder ``start * 2**k`` (``levels_per_call`` levels a call, capped at ``cap``) until a level misses.
  ``lo`` = the last hit below the first miss, ``hi`` = that miss.  A ladder that reaches the cap without a miss returns the
  cap, with a warning.
* REFINE: up to ``levels_per_call`` evenly spaced interior points of ``(lo, hi)`` (never more than it takes to get the gaps
  down to ``resolution``), spaced by the cent-rounded-up step.  New ``lo`` = the largest hit among ``lo`` and the points,
  new ``hi`` = the next evaluated level above it.  Monte Carlo estimates are not monotone in the level, but this keeps
  ``P(lo) >= target > P(hi)`` with ``lo`` and ``hi`` adjacent among the levels evaluated in ``(lo, hi)``.  Stops when
  ``hi - lo <= resolution``: ``ceil(log_{L+1}(range / resolution))`` calls for a resolution of whole cents.

The procedure is a generator (`_search`) that yields the levels a call needs and receives their probabilities, so that
`search_maximum_expenses_many` can run one search per working month in lockstep: each round, every unfinished search's
levels go into ONE rectangular ``probe_rows`` call (the grid probe, `mcr_probe_grid_rng`), and each search sees exactly
the calls it would have made on its own.
"""

from __future__ import annotations

import math
import warnings
from typing import Callable, Dict, Generator, List, Optional, Sequence, Tuple

EXPENSE_CAP = 1e9   # per month


def _cents(x: float) -> int:
    return int(round(round(float(x), 2) * 100))


SearchResult = Tuple[float, float, List[Dict[str, float]]]


def _check(levels_per_call: int, resolution: float) -> None:
    if int(levels_per_call) < 1:
        raise ValueError("levels_per_call must be >= 1")
    if not resolution > 0:
        raise ValueError("resolution must be > 0")


def _search(target: float, start: float, L: int, resolution: float, cap: float,
            on_level: Optional[Callable[[dict], None]]) -> Generator[List[float], Sequence[float], SearchResult]:
    """The search of one working month: yields the levels of a call (1 .. L distinct whole-cent values), receives their
    probabilities, and returns ``(expenses, probability, curve)``."""
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
            curve.append({"monthly_expenses": c / 100.0, "probability": pr})
            if on_level:
                on_level({"type": "expense_search_iter", "iteration": state["call"], "monthly_expenses": c / 100.0,
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
    if memo[0] < target:
        return -1.0, memo[0], curve
    lo, hi, k = 0, None, 0
    while hi is None:
        for c in ladder:
            if c not in memo:
                break
            if memo[c] < target:
                hi = c
                break
            lo = c
        if hi is not None:
            break
        k = next((i for i, c in enumerate(ladder) if c not in memo), None)
        if k is None:   # every rung up to the cap hit
            warnings.warn(f"maximum-spending search reached the cap of {cap:g} per month without missing the target",
                          RuntimeWarning, stacklevel=3)
            return cap_c / 100.0, memo[cap_c], curve
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
        new_lo = max([lo] + hits)
        hi = min(c for c in pts + [hi] if c > new_lo)
        lo = new_lo
        state["lo"], state["hi"] = lo, hi
    return lo / 100.0, memo[lo], curve


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
    _check(levels_per_call, resolution)
    gen = _search(target, start, int(levels_per_call), resolution, cap, on_level)
    try:
        levels = next(gen)
        while True:
            levels = gen.send(probe_levels(levels))
    except StopIteration as done:
        return done.value


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
    _check(levels_per_call, resolution)
    n = len(starts)
    keys = list(range(n)) if working_months is None else [int(m) for m in working_months]
    if len(keys) != n:
        raise ValueError(f"{len(keys)} working months for {n} searches")

    def tagged(i):
        if on_level is None:
            return None
        return lambda ev: on_level(dict(ev, working_months=keys[i]))

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
        width = max(len(pending[i]) for i in rows)
        probs = probe_rows(rows, [pending[i] + [pending[i][-1]] * (width - len(pending[i])) for i in rows])
        if len(probs) != len(rows):
            raise RuntimeError(f"probe_rows returned {len(probs)} rows for {len(rows)}")
        for i, row in zip(rows, probs):
            want = len(pending.pop(i))
            try:
                pending[i] = gens[i].send(list(row)[:want])
            except StopIteration as done:
                results[i] = done.value
    return results  # type: ignore[return-value]
