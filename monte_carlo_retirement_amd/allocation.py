"""Allocation options and the best-split search: how should the money be divided between the two assets?  The question next
to `find_minimum_working_months` (when), `spending.search_maximum_expenses` (how much to spend), `saving`, `nestegg`, `income`
(how much to save, have, receive) and `spending_rules` (which guardrail).

`allocation_records` turns the options a caller writes (a float, or a mapping) into the records of the allocation probes
(``mcr_probe_allocations_rng``: up to ``MCR_MAX_EXPENSE_FANOUT`` splits over the same random numbers).

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
