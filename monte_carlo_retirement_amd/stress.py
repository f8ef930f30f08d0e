"""Market-assumption stress: what the plan's success probability becomes when the market's parameters move, and how far one of
them may move before the target is missed (the margin of safety).

A record of the assumption probe (``mcr_probe_assumptions_rng``) replaces ten fields of the parameter block: the three scenario
levers and the seven lognormal parameters of the market.  Here they are named as `Config` names them (arithmetic annual means and
volatilities, the correlation) and converted with `params.arithmetic_to_log_params`, exactly as `params_from_config` converts the
config itself.  Everything in this module is pure: it runs (and is tested) without a GPU;
`RetirementMonteCarloSimulator.success_probability_by_assumptions`, `.stress_test` and `.find_breakeven_assumption` plug in
the probe, which evaluates up to ``MCR_MAX_EXPENSE_FANOUT`` records over the same random numbers.

Break-even search (`search_breakeven`): the most adverse value of ONE mean or volatility at which the target probability is
still met.  Levels are integer multiples of ``resolution`` (basis points at the default 1e-4) inside ``[base - window, base +
window]`` clipped to the field's `Config` bounds.

* FIRST CALL: both window ends and up to ``levels_per_call - 2`` evenly spaced interior levels.  The adverse end hits ->
  ``"holds_at_window_end"``; no level hits -> ``"not_reached"`` (``None``, with a ``RuntimeWarning``).
* REFINE: `search.refine` on the bracket ``(lo, hi)`` in units of the resolution, ``hi`` the hit on the favourable side and
  ``lo`` the evaluated level next to it on the adverse side.  Stops when ``|hi - lo| <= resolution``: at most ``1 + ceil(log16(2
  window / resolution))`` calls at 15 levels a call.
"""

from __future__ import annotations

import contextlib
import logging
import math
import warnings
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple

from ._logging import logger
from .config import Config
from .nestegg import SCENARIO_FIELDS
from .params import arithmetic_to_log_params
from .search import CALLER, Evaluation, refine, run

#: the `Config` names of the market's assumptions, as (mean, volatility) per series and the correlation
MARKET_FIELDS = (
    "inv1_returns_mean", "inv1_returns_volatility",
    "inflation_rate_mean", "inflation_rate_volatility",
    "inv2_premium_over_inflation_mean", "inv2_premium_over_inflation_volatility",
    "equity_inflation_correlation",
)
#: the keys a record of `assumption_records` may override: the market's seven and the three scenario levers
ASSUMPTION_FIELDS = MARKET_FIELDS + SCENARIO_FIELDS
#: the fields `search_breakeven` takes, with the direction in which they hurt: -1 = lower is adverse, +1 = higher is adverse
ADVERSE_DIRECTION = {
    "inv1_returns_mean": -1, "inv2_premium_over_inflation_mean": -1, "inflation_rate_mean": +1,
    "inv1_returns_volatility": +1, "inflation_rate_volatility": +1, "inv2_premium_over_inflation_volatility": +1,
}
#: lowest arithmetic mean a shift or a search level is clipped to (`Config`: mean > -1)
MEAN_FLOOR = -0.99

#: the default stress table: one-at-a-time additive shifts, (label, {field: delta})
DEFAULT_SHIFTS = (
    ("equity mean -2 pts", {"inv1_returns_mean": -0.02}),
    ("equity mean -1 pt", {"inv1_returns_mean": -0.01}),
    ("equity mean +1 pt", {"inv1_returns_mean": +0.01}),
    ("equity vol +5 pts", {"inv1_returns_volatility": +0.05}),
    ("equity vol -5 pts", {"inv1_returns_volatility": -0.05}),
    ("inflation mean +2 pts", {"inflation_rate_mean": +0.02}),
    ("inflation mean +1 pt", {"inflation_rate_mean": +0.01}),
    ("inflation mean -1 pt", {"inflation_rate_mean": -0.01}),
    ("inflation vol +1 pt", {"inflation_rate_volatility": +0.01}),
    ("premium mean -1 pt", {"inv2_premium_over_inflation_mean": -0.01}),
    ("premium mean +1 pt", {"inv2_premium_over_inflation_mean": +0.01}),
    ("premium vol +2 pts", {"inv2_premium_over_inflation_volatility": +0.02}),
    ("correlation -0.3", {"equity_inflation_correlation": -0.3}),
    ("correlation +0.3", {"equity_inflation_correlation": +0.3}),
)


def field_bounds(field: str) -> Tuple[float, float]:
    """``(lowest, highest)`` value of an assumption field under `Config`'s bounds (means from `MEAN_FLOOR`)."""
    if field not in ASSUMPTION_FIELDS:
        raise ValueError(f"unknown assumption field {field!r}; the fields are {list(ASSUMPTION_FIELDS)}")
    if field == "equity_inflation_correlation":
        return -1.0, 1.0
    if field.endswith("_mean"):
        return MEAN_FLOOR, math.inf
    return 0.0, math.inf     # volatilities and amounts


def clip_to_bounds(field: str, value: float) -> float:
    lo, hi = field_bounds(field)
    return min(max(float(value), lo), hi)


@contextlib.contextmanager
def _soft_checks_muted():
    """`Config`'s two soft volatility checks only warn, once per `Config` built: a record or a search level is validated by
    building one, and a volatility search would print that warning for every level.  The base config has had its own."""
    if isinstance(logger, logging.Logger):
        mute = logging.Filter()
        mute.filter = lambda record: False
        logger.addFilter(mute)
        try:
            yield
        finally:
            logger.removeFilter(mute)
    else:                                   # loguru: by the name of the module that logs
        logger.disable(Config.__module__)
        try:
            yield
        finally:
            logger.enable(Config.__module__)


def assumption_records(config: Config, scenarios: Sequence[Mapping[str, float]]) -> List[tuple]:
    """One 10-tuple in ``mcr_assumptions`` order per mapping of ``scenarios``: ``(initial_balance, monthly_contribution,
    monthly_expenses, inv1 mu_log, sigma_log, inflation mu_log, sigma_log, premium mu_log, sigma_log, rho)``.  A mapping
    overrides any subset of `ASSUMPTION_FIELDS`; a missing key takes the config's value.  Every record is validated by
    building a `Config` from the base with its overrides (pydantic's bounds apply): a ``ValueError`` names ``scenarios[k]``,
    as it does for an unknown key; `Config`'s soft volatility warnings stay silent for the records.  The log parameters are `params_from_config`'s of that `Config`."""
    base = config.model_dump()
    records = []
    for k, s in enumerate(scenarios):
        unknown = sorted(set(s) - set(ASSUMPTION_FIELDS))
        if unknown:
            raise ValueError(f"scenarios[{k}]: unknown key(s) {unknown}; a record may set {list(ASSUMPTION_FIELDS)}")
        if s:
            try:
                with _soft_checks_muted():
                    cfg = Config.model_validate({**base, **{f: float(v) for f, v in s.items()}})
            except ValueError as exc:     # (pydantic's ValidationError is one)
                raise ValueError(f"scenarios[{k}]: {exc}") from exc
        else:
            cfg = config
        m1, s1 = arithmetic_to_log_params(cfg.inv1_returns_mean, cfg.inv1_returns_volatility)
        mi, si = arithmetic_to_log_params(cfg.inflation_rate_mean, cfg.inflation_rate_volatility)
        mp, sp = arithmetic_to_log_params(cfg.inv2_premium_over_inflation_mean, cfg.inv2_premium_over_inflation_volatility)
        records.append((float(cfg.initial_balance), float(cfg.monthly_contribution), float(cfg.monthly_expenses),
                        m1, s1, mi, si, mp, sp, float(cfg.equity_inflation_correlation)))
    return records


def stress_scenarios(config: Config, shifts: Optional[Sequence[Tuple[str, Mapping[str, float]]]] = None) -> List[Tuple[str, Dict[str, float]]]:
    """The rows of a stress table as ``(label, overrides)``: ``("base", {})`` first, then one row per entry of ``shifts``
    (default `DEFAULT_SHIFTS`), whose overrides are the APPLIED values ``config value + delta`` clipped to `Config`'s bounds
    (a volatility shifted below 0 becomes 0).  Several fields in one entry make a combined scenario."""
    rows: List[Tuple[str, Dict[str, float]]] = [("base", {})]
    for k, entry in enumerate(DEFAULT_SHIFTS if shifts is None else shifts):
        try:
            label, deltas = entry
            deltas = dict(deltas)
        except (TypeError, ValueError):
            raise ValueError(f"shifts[{k}]: expected (label, {{field: delta, ...}})") from None
        unknown = sorted(set(deltas) - set(ASSUMPTION_FIELDS))
        if unknown:
            raise ValueError(f"shifts[{k}]: unknown field(s) {unknown}; a shift may move {list(ASSUMPTION_FIELDS)}")
        rows.append((str(label), {f: clip_to_bounds(f, float(getattr(config, f)) + float(d)) for f, d in deltas.items()}))
    return rows


BreakevenResult = Tuple[Optional[float], float, List[Dict[str, float]], str]


def search_breakeven(
    probe_levels: Callable[[Sequence[float]], Sequence[float]],
    target: float,
    field: str,
    base: float,
    window: float = 0.25,
    resolution: float = 1e-4,
    levels_per_call: int = 15,
    on_level: Optional[Callable[[dict], None]] = None,
) -> BreakevenResult:
    """Returns ``(value, probability, curve, status)``: the most adverse level of ``field`` found with ``P >= target``, its
    probability, ``{"value", "probability"}`` per evaluated level in evaluation order, and ``"found"``,
    ``"holds_at_window_end"`` (the adverse end of the window still hits: the value is that end) or ``"not_reached"`` (no
    level of the window hits: ``None`` and the probability of the favourable end, with a ``RuntimeWarning``).
    ``probe_levels(values) -> [success %]`` evaluates values of ``field``; ``on_level`` receives one
    ``"breakeven_search_iter"`` event per evaluated level."""
    if field not in ADVERSE_DIRECTION:
        raise ValueError(f"break-even search: field {field!r} is not one of {sorted(ADVERSE_DIRECTION)}")
    L = int(levels_per_call)
    if L < 3:
        raise ValueError("levels_per_call must be >= 3")
    if not (resolution > 0 and math.isfinite(resolution)) or not (window > 0 and math.isfinite(window)):
        raise ValueError("window and resolution must be positive and finite")
    res = float(resolution)
    lo_v, hi_v = field_bounds(field)
    lo_v, hi_v = max(lo_v, float(base) - float(window)), min(hi_v, float(base) + float(window))
    k_min, k_max = math.ceil(lo_v / res - 1e-9), math.floor(hi_v / res + 1e-9)     # levels are k * resolution
    if k_min > k_max:
        raise ValueError(f"break-even search: no multiple of {res:g} in [{lo_v:g}, {hi_v:g}]")
    # t runs from the adverse end (smallest) to the favourable end: success rises with t, and the answer is the smallest t that hits
    sign = -ADVERSE_DIRECTION[field]              # k = sign * t
    t_min, t_max = sorted((sign * k_min, sign * k_max))

    def value_of(t: int) -> float:
        return round(sign * t * res, 12)

    ev = Evaluation(value_of, "value", "breakeven_search_iter", target, on_level, {"field": field})
    memo = ev.memo

    def steps():
        # first call: both ends and evenly spaced interior levels
        span = t_max - t_min
        n_int = min(L - 2, max(0, span - 1))
        first = sorted({t_min, t_max, *(t_min + (i * span) // (n_int + 1) for i in range(1, n_int + 1))})
        yield from ev.evaluate(first)
        if ev.hit(t_min):
            return value_of(t_min), memo[t_min], ev.curve, "holds_at_window_end"
        hits = [t for t in first if ev.hit(t)]
        if not hits:
            ends = sorted((value_of(t_min), value_of(t_max)))
            warnings.warn(f"break-even search: no value of {field} in [{ends[0]:g}, {ends[1]:g}] reaches the target",
                          RuntimeWarning, stacklevel=CALLER)
            return None, memo[t_max], ev.curve, "not_reached"
        hi = min(hits)
        hi = yield from refine(ev, max(t for t in first if t < hi), hi, L, 1, largest=False)
        return value_of(hi), memo[hi], ev.curve, "found"

    return run(steps(), probe_levels)
