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
"""

from __future__ import annotations

import math
import warnings
from typing import Callable, Dict, List, Optional, Sequence, Tuple

EXPENSE_CAP = 1e9   # per month


def _cents(x: float) -> int:
    return int(round(round(float(x), 2) * 100))


def search_maximum_expenses(
    probe_levels: Callable[[Sequence[float]], Sequence[float]],
    target: float,
    start: float,
    levels_per_call: int = 15,
    resolution: float = 1.0,
    cap: float = EXPENSE_CAP,
    on_level: Optional[Callable[[dict], None]] = None,
) -> Tuple[float, float, List[Dict[str, float]]]:
    """Returns ``(expenses, probability, curve)``: the largest level found with ``P >= target`` (``-1.0`` when even zero
    spending misses), its probability, and ``{"monthly_expenses", "probability"}`` per evaluated level in evaluation order.
    ``on_level`` receives one ``"expense_search_iter"`` event per evaluated level."""
    L = int(levels_per_call)
    if L < 1:
        raise ValueError("levels_per_call must be >= 1")
    if not resolution > 0:
        raise ValueError("resolution must be > 0")
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
    evaluate([0] + ladder[: L - 1])
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
                          RuntimeWarning, stacklevel=2)
            return cap_c / 100.0, memo[cap_c], curve
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
        new_lo = max([lo] + hits)
        hi = min(c for c in pts + [hi] if c > new_lo)
        lo = new_lo
        state["lo"], state["hi"] = lo, hi
    return lo / 100.0, memo[lo], curve
