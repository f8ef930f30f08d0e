"""The one level search behind every planning question that asks "how much": `spending` (the most one can spend), `saving`,
`nestegg`, `income` (the least one must save, have, receive) and `stress.search_breakeven` (how far an assumption may move).

A search is a pure function of a probe ``levels -> [success %]`` and runs (and is tested) without a GPU.  It is written as a
generator that yields the levels of a call and receives their probabilities, so that one search (`run`) and many searches in
lockstep (`run_many`) are driven by the same code and each search sees exactly the calls it would have made on its own.

Levels are integers (UNITS) internally: whole cents for the four amount searches, multiples of the resolution for break-even.

* `Evaluation` asks for the levels not yet known, keeps the memo and the curve, and emits one event per evaluated level.
* `cent_search` BRACKETS with a geometric ladder ``start * 2**k`` (``L`` levels a call, capped at ``cap``; ``P(0)`` goes with the
  first rungs) and hands the bracket to `refine`.  A MINIMUM search returns ``0.0`` when ``P(0)`` hits, climbs until a rung hits
  (``hi`` = that hit, ``lo`` = the last miss below it) and returns ``-1.0`` with a warning when the ladder reaches the cap without
  one.  A MAXIMUM search (``largest``) returns ``-1.0`` when ``P(0)`` misses, climbs until a rung misses (``lo`` = the last hit,
  ``hi`` = that miss) and returns the cap with a warning when none does.
* `refine` REFINES ``(lo, hi)``: up to ``L`` evenly spaced interior points (never more than it takes to get the gaps down to the
  resolution), spaced by the step rounded up to a whole unit.  Minimum: new ``hi`` = the smallest hit among the points and
  ``hi``, new ``lo`` = the largest evaluated level below it; maximum: the mirror image.  Monte Carlo estimates are not monotone in
  the level, but this keeps one end hitting and the other missing, adjacent among the levels evaluated in ``(lo, hi)``.  Stops
  when ``hi - lo <= resolution``: ``ceil(log_{L+1}(range / resolution))`` calls for a resolution of whole units.

Warnings are raised with ``stacklevel=4``: generator, driver, public search function, and the caller it is attributed to.
"""

from __future__ import annotations

import math
import warnings
from typing import Callable, Dict, Generator, List, Mapping, Optional, Sequence, Tuple

SearchResult = Tuple[float, float, List[Dict[str, float]]]
Steps = Generator[List[float], Sequence[float], tuple]
CALLER = 4      # the stacklevel of a warning raised in a search generator that `run` / `run_many` drives from a public function


def cents(x: float) -> int:
    return int(round(round(float(x), 2) * 100))


def check(levels_per_call: int, resolution: float) -> None:
    if int(levels_per_call) < 1:
        raise ValueError("levels_per_call must be >= 1")
    if not resolution > 0:
        raise ValueError("resolution must be > 0")


class Evaluation:
    """What a search knows: ``memo[unit]``, the ``curve`` in evaluation order, and the bracket the events report."""

    def __init__(self, value_of: Callable[[int], float], key: str, event: str, target: float,
                 on_level: Optional[Callable[[dict], None]], extra: Optional[Mapping[str, object]] = None):
        self.value_of, self.key, self.target, self.on_level = value_of, key, target, on_level
        self.head = {"type": event, **(extra or {})}
        self.memo: Dict[int, float] = {}
        self.curve: List[Dict[str, float]] = []
        self.call, self.lo, self.hi = 0, None, None

    def hit(self, unit: int) -> bool:
        return self.memo[unit] >= self.target

    def evaluate(self, units: List[int]):
        """Yields the values of the distinct units not yet in the memo (one call, if there are any) and records the answers."""
        units = [u for u in dict.fromkeys(units) if u not in self.memo]
        if not units:
            return
        self.call += 1
        value_of = self.value_of
        probs = list((yield [value_of(u) for u in units]))
        if len(probs) != len(units):
            raise RuntimeError(f"probe_levels returned {len(probs)} values for {len(units)} levels")
        for u, pr in zip(units, probs):
            pr = float(pr)
            self.memo[u] = pr
            self.curve.append({self.key: value_of(u), "probability": pr})
            if self.on_level:
                self.on_level({**self.head, "iteration": self.call, self.key: value_of(u), "probability": round(pr, 2),
                               "target": self.target, "lo": None if self.lo is None else value_of(self.lo),
                               "hi": None if self.hi is None else value_of(self.hi)})


def refine(ev: Evaluation, lo: int, hi: int, L: int, resolution: float, largest: bool):
    """Narrows the bracket ``(lo, hi)`` to ``resolution`` units and returns the answer's unit: the smallest hit (``hi``), or
    with ``largest`` the largest (``lo``)."""
    ev.lo, ev.hi = lo, hi
    while hi - lo > resolution:
        w = hi - lo
        n_pts = min(L, max(1, math.ceil(w / resolution) - 1), w - 1)
        step = -(-w // (n_pts + 1))     # (units, rounded up: the largest gap is the step)
        pts = [lo + i * step for i in range(1, n_pts + 1) if lo + i * step < hi]
        if not pts:
            break
        yield from ev.evaluate(pts)
        hits = [u for u in pts if ev.hit(u)]
        if largest:
            lo = max([lo] + hits)
            hi = min(u for u in pts + [hi] if u > lo)
        else:
            hi = min([hi] + hits)
            lo = max(u for u in pts + [lo] if u < hi)
        ev.lo, ev.hi = lo, hi
    return lo if largest else hi


def cent_search(target: float, start: float, L: int, resolution: float, cap: float, on_level: Optional[Callable[[dict], None]],
                *, largest: bool, key: str, event: str, cap_warning: str) -> Steps:
    """One search over whole cents: yields the levels of a call (1 .. L distinct values), receives their probabilities, and
    returns ``(level, probability, curve)``.  ``key`` names the level in the curve and the events, ``event`` is the events' type."""
    cap_c = cents(cap)
    ev = Evaluation(lambda c: c / 100.0, key, event, target, on_level)
    memo = ev.memo
    # bracket: 0 and the first rungs in one call, then L rungs a call
    rung = max(cents(max(float(start), 1.0)), 1)
    ladder: List[int] = []
    while True:
        ladder.append(min(rung, cap_c))
        if rung >= cap_c:
            break
        rung *= 2
    yield from ev.evaluate([0] + ladder[: L - 1])
    if ev.hit(0) != largest:            # nothing is needed / even nothing is too much
        return (-1.0 if largest else 0.0), memo[0], ev.curve
    lo, hi = 0, None
    while hi is None:
        for c in ladder:
            if c not in memo:
                break
            if ev.hit(c) != largest:    # the first hit / the first miss ends the bracket
                hi = c
                break
            lo = c
        if hi is not None:
            break
        k = next((i for i, c in enumerate(ladder) if c not in memo), None)
        if k is None:                   # every rung up to the cap missed / hit
            warnings.warn(cap_warning, RuntimeWarning, stacklevel=CALLER)
            return (cap_c / 100.0 if largest else -1.0), memo[cap_c], ev.curve
        yield from ev.evaluate(ladder[k: k + L])
    best = yield from refine(ev, lo, hi, L, float(resolution) * 100.0, largest)
    return best / 100.0, memo[best], ev.curve


def run(steps: Steps, probe_levels: Callable[[Sequence[float]], Sequence[float]]) -> tuple:
    """Drives one search to its result."""
    try:
        levels = next(steps)
        while True:
            levels = steps.send(probe_levels(levels))
    except StopIteration as done:
        return done.value


def run_many(make_steps: Callable[[int, Optional[Callable[[dict], None]]], Steps], n: int,
             probe_rows: Callable[[List[int], List[List[float]]], Sequence[Sequence[float]]], pad: bool,
             on_level: Optional[Callable[[dict], None]] = None, tag: Optional[Callable[[int], dict]] = None) -> List[tuple]:
    """Drives ``make_steps(i, on_level_i)`` for ``i < n`` in lockstep.  Each round calls ``probe_rows(rows, levels_2d)`` once:
    ``rows`` are the indices of the unfinished searches, ``levels_2d`` their next levels.  With ``pad`` every row is padded to
    the widest by repeating its own last level, and the padded results are discarded; without, rows differ in length.  Search
    ``i``'s events also carry the fields of ``tag(i)``, when a tagger is given."""
    def tagged(i):
        if on_level is None or tag is None:
            return on_level
        return lambda ev: on_level(dict(ev, **tag(i)))

    gens = [make_steps(i, tagged(i)) for i in range(n)]
    results: List[Optional[tuple]] = [None] * n
    pending: Dict[int, List[float]] = {}
    for i, g in enumerate(gens):
        try:
            pending[i] = next(g)
        except StopIteration as done:
            results[i] = done.value
    while pending:
        rows = sorted(pending)
        width = max(len(pending[i]) for i in rows)
        probs = probe_rows(rows, [pending[i] + [pending[i][-1]] * (width - len(pending[i]) if pad else 0) for i in rows])
        if len(probs) != len(rows):
            raise RuntimeError(f"probe_rows returned {len(probs)} rows for {len(rows)}")
        for i, row in zip(rows, probs):
            want = len(pending.pop(i))
            try:
                pending[i] = gens[i].send(list(row)[:want] if pad else list(row))
            except StopIteration as done:
                results[i] = done.value
    return results  # type: ignore[return-value]
