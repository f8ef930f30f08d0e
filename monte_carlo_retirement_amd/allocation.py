"""Allocation options and the best-split search: how should the money be divided between the two assets?  The question next
to `find_minimum_working_months` (when), `spending.search_maximum_expenses` (how much to spend), `saving`, `nestegg`, `income`
(how much to save, have, receive) and `spending_rules` (which guardrail).

`allocation_records` turns the options a caller writes (a float, or a mapping) into the records of the allocation probes
(``mcr_probe_allocations_rng``: up to ``MCR_MAX_EXPENSE_FANOUT`` splits over the same random numbers).

`GlidePath` is a split that changes with the calendar (a table of weights by whole years from today) and `glide_records` builds
the records of the glide probes (``mcr_probe_glide_paths_rng``) from the glide options a caller writes.

`search_best_allocation` is a pure function of a ``probe_levels(splits) -> [success %]`` callable, so it runs (and is tested)
without a GPU.  Success as a function of the split is NOT monotone (too little of the growth asset starves the plan, too much
exposes it), so nothing of `search.cent_search` or `search.refine` applies: the search keeps `search.Evaluation` (memo, curve,
events) and refines a GRID around the best point seen.  Every round probes the same paths, so the objective is a fixed integer
function of the split and the search is deterministic.
"""

from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

from .nestegg import SCENARIO_FIELDS
from .search import Evaluation, check, run

#: the keys an allocation option may set, in record order (``mcr_allocation_option``)
ALLOCATION_OPTION_FIELDS = SCENARIO_FIELDS + ("allocation_inv1_pct",)

#: the splits `RetirementMonteCarloSimulator.compare_allocations` compares by default, and round 1 of the search
DEFAULT_ALLOCATIONS = tuple(i / 10.0 for i in range(11))

AllocationResult = Tuple[float, float, List[Dict[str, float]], List[float]]


def allocation_records(p, options: Sequence) -> List[tuple]:
    """``(initial_balance, monthly_contribution, monthly_expenses, allocation_inv1_pct)`` per entry of ``options``.  An option
    is a number (the split; the three amounts are the config's) or a mapping with ``allocation_inv1_pct`` and any subset of the
    three scenario keys (a missing amount takes the config's value).  ``p`` is the config (`config.Config`).  Raises
    ``ValueError`` naming the option and the field: an unknown key, a mapping without a split, an amount that is not finite and
    >= 0, a split that is not finite and in [0, 1]."""
    defaults = (float(p.initial_balance), float(p.monthly_contribution), float(p.monthly_expenses))
    records = []
    for k, o in enumerate(options):
        if isinstance(o, dict):
            unknown = sorted(set(o) - set(ALLOCATION_OPTION_FIELDS))
            if unknown:
                raise ValueError(f"allocations[{k}]: unknown key(s) {unknown}; an option may set {list(ALLOCATION_OPTION_FIELDS)}")
            if "allocation_inv1_pct" not in o:
                raise ValueError(f"allocations[{k}].allocation_inv1_pct is missing")
            values = [o.get(f, d) for f, d in zip(SCENARIO_FIELDS, defaults)] + [o["allocation_inv1_pct"]]
        else:
            values = list(defaults) + [o]
        record = []
        for f, v in zip(ALLOCATION_OPTION_FIELDS, values):
            try:
                x = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"allocations[{k}].{f} = {v!r}: must be a number") from None
            if f == "allocation_inv1_pct":
                if not (math.isfinite(x) and 0.0 <= x <= 1.0):
                    raise ValueError(f"allocations[{k}].{f} = {x!r}: must be finite and in [0, 1]")
            elif not (math.isfinite(x) and x >= 0.0):
                raise ValueError(f"allocations[{k}].{f} = {x!r}: must be finite and >= 0")
            record.append(x)
        records.append(tuple(record))
    return records


def _steps(own: float, L: int, resolution: float, on_level: Optional[Callable[[dict], None]]):
    """The search's generator, in UNITS of the resolution (split = unit * resolution, 0 .. n_units)."""
    n_units = int(round(1.0 / resolution))
    if n_units < 1 or abs(n_units * resolution - 1.0) > 1e-9:
        raise ValueError(f"resolution {resolution!r}: 1 / resolution must be a whole number")

    def value_of(u: int) -> float:
        return round(u * resolution, 12)

    def drop_target(event: dict) -> None:       # (a maximisation has no target: Evaluation's event without that key)
        on_level({k: v for k, v in event.items() if k != "target"})

    ev = Evaluation(value_of, "allocation_inv1_pct", "allocation_search_iter", -math.inf, drop_target if on_level else None)

    own_u = own / resolution

    def best_unit() -> int:                      # highest probability; then nearest the config's own split; then the lower
        # (distances in units of the resolution, rounded far below one unit and far above the rounding of own / resolution:
        # two points equally far from the config's split compare equal, whatever their last bits)
        return min(ev.memo, key=lambda u: (-ev.memo[u], round(abs(u - own_u), 6), u))

    def evaluate(units: List[int]):
        units = [u for u in dict.fromkeys(units) if u not in ev.memo]
        for i in range(0, len(units), L):        # (one call a round unless a caller asks for fewer levels than a round has)
            yield from ev.evaluate(units[i:i + L])

    grid = list(dict.fromkeys(int(round(n_units * i / 10.0)) for i in range(11)))      # round 1: 0, 0.1, ..., 1
    yield from evaluate(grid)
    step = max(1, -(-n_units // 10))
    while step > 1:
        best = best_unit()
        # the coarsest step whose points inside (best - step, best + step) fit one probe, and never more than half the step (L = 1,
        # 2: a probe holds less than one point a side, so the step must shrink on its own; `evaluate` then splits the round)
        finer = max(1, min(-(-2 * step // (L + 1)), -(-step // 2)))
        ev.lo, ev.hi = max(0, best - step), min(n_units, best + step)
        reach = -(-step // finer) - 1                    # points a side, strictly inside the bracket
        yield from evaluate([u for k in range(1, reach + 1) for u in (best - k * finer, best + k * finer) if 0 <= u <= n_units])
        step = finer
    best = best_unit()
    return best, ev, grid, value_of


def search_best_allocation(
    probe_levels: Callable[[Sequence[float]], Sequence[float]],
    own_allocation: float,
    resolution: float = 0.01,
    levels_per_call: int = 15,
    on_level: Optional[Callable[[dict], None]] = None,
    probe_joint: Optional[Callable[[Sequence[float]], object]] = None,
) -> AllocationResult:
    """The split with the highest success probability among the points of a refined grid.  Returns ``(allocation_inv1_pct,
    probability, curve, tied)``.

    Round 1 probes 0, 0.1, ..., 1; each later round probes a finer grid strictly inside ``(best - step, best + step)``, clipped
    to [0, 1], around the best point so far, in one ``probe_levels`` call of at most ``levels_per_call`` new points (with fewer
    than 11 levels a call a round takes several calls, and with 1 or 2 the step halves from round to round): for the default
    resolution the steps are 0.1 -> 0.02 -> 0.01, three calls.  Every point is a multiple of ``resolution`` (whose
    reciprocal must be a whole number) and no point is probed twice.  The answer is the best of ALL evaluated points; ties go to
    the point nearest ``own_allocation`` (the config's split: no reason to move), then to the lower.  ``curve`` holds
    ``{"allocation_inv1_pct", "probability"}`` per evaluated point in evaluation order; ``on_level`` receives one
    ``{"type": "allocation_search_iter", "iteration", "allocation_inv1_pct", "probability", "lo", "hi"}`` event per point
    (``lo`` / ``hi``: the bracket being refined, None in round 1).

    A grid refinement CANNOT promise the global optimum of a noisy, possibly multi-modal curve: a peak narrower than the grid
    it falls through is missed, and near a flat top the differences are Monte Carlo noise.  To qualify the answer the search
    ends with one JOINT probe, ``probe_joint(splits)`` -> a `paired.JointOutcomes` over the round-1 grid plus the answer on the
    same paths: ``tied`` holds the splits of that probe the paired test cannot tell from the answer (the answer included) --
    the plateau a user may choose from on other grounds.  Without ``probe_joint``, ``tied`` is the answer alone."""
    check(levels_per_call, resolution)
    if not (math.isfinite(float(own_allocation)) and 0.0 <= float(own_allocation) <= 1.0):
        raise ValueError(f"own_allocation = {own_allocation!r}: must be finite and in [0, 1]")
    best, ev, grid, value_of = run(_steps(float(own_allocation), int(levels_per_call), float(resolution), on_level), probe_levels)
    answer = value_of(best)
    tied = [answer]
    if probe_joint is not None:
        units = sorted(set(grid) | {best})
        joint = probe_joint([value_of(u) for u in units])
        tied = [value_of(units[j]) for j in joint.indistinguishable_from(units.index(best))]
    return answer, ev.memo[best], ev.curve, tied


# ---- glide paths: a split that changes with the calendar (include/mcr.h: GLIDE PATH) ------------------------------------

#: the keys a glide option given as a mapping may set
GLIDE_OPTION_FIELDS = SCENARIO_FIELDS + ("glide_path",)


def _weight(x, what: str) -> float:
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{what} = {x!r}: must be a number") from None
    if not (math.isfinite(v) and 0.0 <= v <= 1.0):
        raise ValueError(f"{what} = {v!r}: must be finite and in [0, 1]")
    return v


def _year(x, what: str) -> int:
    if isinstance(x, bool) or int(x) != x or int(x) < 0:
        raise ValueError(f"{what} = {x!r}: must be a whole number of years >= 0")
    return int(x)


class GlidePath:
    """An immutable table of ``allocation_inv1_pct`` values indexed by WHOLE YEARS FROM TODAY: entry ``y`` is in force during
    months ``12 y .. 12 y + 11`` from today, whatever the retirement month; a table shorter than the horizon holds its last
    entry, entries past the horizon are never read.  Every entry is finite and in [0, 1]; there is at least one."""

    __slots__ = ("_weights", "_name")

    def __init__(self, weights: Sequence[float], name: Optional[str] = None):
        try:
            entries = list(weights)
        except TypeError:
            raise ValueError(f"glide path weights = {weights!r}: must be a sequence of numbers") from None
        if not entries:
            raise ValueError("a glide path has at least one weight")
        object.__setattr__(self, "_weights", tuple(_weight(w, f"weights[{i}]") for i, w in enumerate(entries)))
        object.__setattr__(self, "_name", None if name is None else str(name))

    def __setattr__(self, key, value):
        raise AttributeError("a GlidePath is immutable")

    @property
    def weights(self) -> Tuple[float, ...]:
        return self._weights

    @property
    def name(self) -> Optional[str]:
        return self._name

    def named(self, name: str) -> "GlidePath":
        return GlidePath(self._weights, name)

    def weight_at(self, month_from_today: int) -> float:
        """The weight in force while 0-based month ``month_from_today`` is processed: ``W[min(t // 12, n - 1)]``."""
        if month_from_today < 0:
            raise ValueError("month_from_today must be >= 0")
        return self._weights[min(int(month_from_today) // 12, len(self._weights) - 1)]

    def __len__(self) -> int:
        return len(self._weights)

    def __eq__(self, other) -> bool:
        return isinstance(other, GlidePath) and self._weights == other._weights

    def __hash__(self) -> int:
        return hash(self._weights)

    def __repr__(self) -> str:
        return f"GlidePath({self.describe()})"

    @classmethod
    def constant(cls, allocation: float, name: Optional[str] = None) -> "GlidePath":
        """The constant split ``allocation``: a table of one entry."""
        return cls([_weight(allocation, "allocation")], name)

    @classmethod
    def linear(cls, start: float, end: float, from_year: int, to_year: int, name: Optional[str] = None) -> "GlidePath":
        """``start`` up to and including year ``from_year``, ``end`` from year ``to_year`` on, and a straight line between them:
        ``to_year + 1`` entries (``from_year == to_year``: a step to ``end`` in the year after)."""
        a, b = _weight(start, "start"), _weight(end, "end")
        y0, y1 = _year(from_year, "from_year"), _year(to_year, "to_year")
        if y1 < y0:
            raise ValueError(f"to_year = {y1} < from_year = {y0}")
        if y1 == y0:
            return cls([a] * (y0 + 1) + [b], name)
        table = []
        for y in range(y1 + 1):
            if y <= y0:
                table.append(a)
            elif y >= y1:
                table.append(b)
            else:
                table.append(min(1.0, max(0.0, a + (b - a) * ((y - y0) / (y1 - y0)))))
        return cls(table, name)

    @classmethod
    def around_retirement(cls, working_months: int, before: float, at: float, after: float, years_before: int, years_after: int,
                          name: Optional[str] = None) -> "GlidePath":
        """The target-date and the rising-equity shapes, in years from today for a retirement after ``working_months``:
        ``before`` until ``years_before`` years ahead of the retirement year ``R = working_months // 12``, a straight line to
        ``at`` in year ``R``, a straight line to ``after`` in year ``R + years_after``, ``after`` from then on.  A line that
        would begin before today begins today, at the value it has there."""
        wm = _year(working_months, "working_months")
        w0, w1, w2 = _weight(before, "before"), _weight(at, "at"), _weight(after, "after")
        yb, ya = _year(years_before, "years_before"), _year(years_after, "years_after")
        r = wm // 12
        table = []
        for y in range(r + ya + 1):
            if y <= r:
                x = w1 if yb == 0 and y == r else w0 if y <= r - yb else w0 + (w1 - w0) * ((y - (r - yb)) / yb)
            else:
                x = w2 if ya == 0 else w1 + (w2 - w1) * ((y - r) / ya)
            table.append(min(1.0, max(0.0, x)))
        return cls(table, name)

    @classmethod
    def parse(cls, text: str) -> "GlidePath":
        """``"0.6"`` (a constant) or ``"start>end@from-to"`` (`linear`), the command-line tool's syntax."""
        t = str(text).strip()
        try:
            if ">" not in t:
                return cls.constant(float(t), t)
            levels, _, years = t.partition("@")
            start, _, end = levels.partition(">")
            y0, _, y1 = years.partition("-")
            return cls.linear(float(start), float(end), int(y0), int(y1), t)
        except ValueError as e:
            raise ValueError(f"glide path {text!r}: expected a constant or start>end@from-to ({e})") from None

    def describe(self) -> str:
        """A short description: the name where there is one, else the run-length form of the table."""
        if self._name:
            return self._name
        w = self._weights
        if all(x == w[0] for x in w):
            return f"constant {w[0]:.4g}"
        return f"{w[0]:.4g} -> {w[-1]:.4g} over {len(w)} years"


def default_glide_paths(p, working_months: int) -> List[GlidePath]:
    """The catalogue `RetirementMonteCarloSimulator.compare_glide_paths` compares when it is given no list, built for a
    retirement after ``working_months``: the config's own constant split, all of asset 1, none of it, two declining target-date
    shapes and one rising-equity shape."""
    wm = int(working_months)
    return [
        GlidePath.constant(float(p.allocation_inv1_pct), "own constant split"),
        GlidePath.constant(1.0, "all in asset 1"),
        GlidePath.constant(0.0, "all in asset 2"),
        GlidePath.around_retirement(wm, 0.9, 0.5, 0.4, 20, 10, "target date 90 > 50 > 40"),
        GlidePath.around_retirement(wm, 0.8, 0.6, 0.3, 15, 15, "target date 80 > 60 > 30"),
        GlidePath.around_retirement(wm, 0.6, 0.3, 0.6, 10, 15, "rising equity 60 > 30 > 60"),
    ]


def glide_paths_of(options: Sequence) -> List[GlidePath]:
    """The `GlidePath` of every entry of ``options`` (see `glide_records`), validated."""
    paths = []
    for k, o in enumerate(options):
        try:
            if isinstance(o, dict):
                if "glide_path" not in o:
                    raise ValueError("glide_path is missing")
                o = o["glide_path"]
            if isinstance(o, GlidePath):
                paths.append(o)
            elif isinstance(o, (int, float)) and not isinstance(o, bool):
                paths.append(GlidePath.constant(o))
            elif isinstance(o, str):
                paths.append(GlidePath.parse(o))
            else:
                paths.append(GlidePath(o))
        except ValueError as e:
            raise ValueError(f"glide_paths[{k}]: {e}") from None
    return paths


def glide_records(p, options: Sequence) -> Tuple[List[tuple], List[float]]:
    """``(records, table)`` of the glide probes (``mcr_probe_glide_paths_rng``): ``records[k] = (initial_balance,
    monthly_contribution, monthly_expenses, first_weight, n_weights)`` and ``table`` the flat list of all options' weights,
    option k's at ``table[first_weight : first_weight + n_weights]`` (equal tables are stored once).  An option is a
    `GlidePath`, a sequence of weights, a number (a constant split), a string in `GlidePath.parse`'s syntax, or a mapping with
    ``glide_path`` (any of those) and any subset of the three scenario keys (a missing amount takes the config's value).
    ``p`` is the config.  Raises ``ValueError`` naming the option and the field, as `allocation_records` does."""
    defaults = (float(p.initial_balance), float(p.monthly_contribution), float(p.monthly_expenses))
    for k, o in enumerate(options):
        if isinstance(o, dict):
            unknown = sorted(set(o) - set(GLIDE_OPTION_FIELDS))
            if unknown:
                raise ValueError(f"glide_paths[{k}]: unknown key(s) {unknown}; an option may set {list(GLIDE_OPTION_FIELDS)}")
            if "glide_path" not in o:
                raise ValueError(f"glide_paths[{k}].glide_path is missing")
    paths = glide_paths_of(options)
    records, table, first_of = [], [], {}
    for k, (o, path) in enumerate(zip(options, paths)):
        amounts = []
        for f, d in zip(SCENARIO_FIELDS, defaults):
            v = o.get(f, d) if isinstance(o, dict) else d
            try:
                x = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"glide_paths[{k}].{f} = {v!r}: must be a number") from None
            if not (math.isfinite(x) and x >= 0.0):
                raise ValueError(f"glide_paths[{k}].{f} = {x!r}: must be finite and >= 0")
            amounts.append(x)
        if path.weights not in first_of:
            first_of[path.weights] = len(table)
            table.extend(path.weights)
        records.append((*amounts, first_of[path.weights], len(path.weights)))
    return records, table
