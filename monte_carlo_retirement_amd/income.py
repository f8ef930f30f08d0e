"""Income-stream options and the required-income search: what `other_income_streams` raises as planning questions — claim
at 62, 67 or 70 (the amount differs at each age), how large an annuity or a part-time income has to be, whether turning part
of the balance into a monthly payment for life is worth it, what a bridge job of three years instead of five does.  Next to
`find_minimum_working_months` (when), `spending.search_maximum_expenses` (how much to spend),
`saving.search_minimum_contribution` (how much to save), `nestegg.search_minimum_initial_balance` (how much to have) and
`stress.search_breakeven` (what if the market does worse).

An OPTION is one version of ONE stream of the config's list, together with the three scenario levers (so that "200 000 of the
balance for 1 100 a month" is one option): the six fields of `INCOME_OPTION_FIELDS`.  The stream's ``tax_rate`` and
``inflation_indexed`` stay the list's own.  `RetirementMonteCarloSimulator.success_probability_by_income_options` evaluates
up to ``MCR_MAX_EXPENSE_FANOUT`` options over the same random numbers (`mcr_probe_income_rng`).

The search is a pure function of a ``probe_levels(levels) -> [success %]`` callable, so it runs (and is tested) without a
GPU.  Its procedure is `nestegg`'s (`search.cent_search`), with the level's key and the event name passed in.
"""

from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Union

from .nestegg import _steps
from .search import SearchResult, check, run

#: Highest monthly amount the search tries: `saving.CONTRIBUTION_CAP`'s headroom argument, for money that flows the other
#: way.  An income of 1e8 a month offsets that much spending; a plan whose target such an income does not reach fails before
#: the income starts, and is not reached by a larger one.
INCOME_AMOUNT_CAP = 1e8

#: the keys an option mapping may set, in the order of ``mcr_income_option``
INCOME_OPTION_FIELDS = ("initial_balance", "monthly_contribution", "monthly_expenses", "monthly_amount_today", "start_at_age",
                        "duration_years")


def stream_index(config, stream: Union[int, str]) -> int:
    """The list index of ``stream`` in ``config.other_income_streams``: an index as it is (checked against the list), a
    ``name`` when exactly one stream carries it; otherwise ``ValueError``."""
    streams = list(config.other_income_streams)
    if isinstance(stream, str):
        hits = [i for i, s in enumerate(streams) if s.name == stream]
        if not hits:
            raise ValueError(f"no income stream is named {stream!r}; the config has {[s.name for s in streams]}")
        if len(hits) > 1:
            raise ValueError(f"income stream name {stream!r} is ambiguous: entries {hits} carry it; pass the list index")
        return hits[0]
    if isinstance(stream, bool) or int(stream) != stream:
        raise ValueError(f"stream must be a list index or a name, not {stream!r}")
    i = int(stream)
    if not 0 <= i < len(streams):
        raise ValueError(f"stream index {i} is outside the config's {len(streams)} income stream(s)")
    return i


def income_options(config, stream: Union[int, str], options: Sequence[dict]) -> List[tuple]:
    """``(initial_balance, monthly_contribution, monthly_expenses, monthly_amount_today, start_at_age, duration_years)`` per
    mapping of ``options``, for `engine.probe_income`: a missing key takes the config's own value (of stream ``stream`` for
    the last three), an unknown key raises ``ValueError`` naming it.  ``duration_years`` is an int or ``None`` (for life)."""
    own = config.other_income_streams[stream_index(config, stream)]
    defaults = (config.initial_balance, config.monthly_contribution, config.monthly_expenses, own.monthly_amount_today,
                own.start_at_age, own.duration_years)
    records = []
    for k, o in enumerate(options):
        unknown = sorted(set(o) - set(INCOME_OPTION_FIELDS))
        if unknown:
            raise ValueError(f"options[{k}]: unknown key(s) {unknown}; an option may set {list(INCOME_OPTION_FIELDS)}")
        five = tuple(float(o.get(f, d)) for f, d in zip(INCOME_OPTION_FIELDS[:5], defaults))
        duration = o.get("duration_years", defaults[5])
        if duration is not None and (isinstance(duration, bool) or int(duration) != duration or duration < 0):
            raise ValueError(f"options[{k}]: duration_years must be a whole number of years >= 0 or None, not {duration!r}")
        records.append(five + (None if duration is None else int(duration),))
    return records


def search_minimum_income_amount(
    probe_levels: Callable[[Sequence[float]], Sequence[float]],
    target: float,
    start: float,
    levels_per_call: int = 15,
    resolution: float = 1.0,
    cap: float = INCOME_AMOUNT_CAP,
    on_level: Optional[Callable[[dict], None]] = None,
) -> SearchResult:
    """Returns ``(monthly_amount_today, probability, curve)``: the smallest level found with ``P >= target`` (``0.0`` when no
    income is needed, ``-1.0`` with a ``RuntimeWarning`` when even ``cap`` misses), its probability, and
    ``{"monthly_amount_today", "probability"}`` per evaluated level in evaluation order.  ``on_level`` receives one
    ``"income_amount_search_iter"`` event per evaluated level."""
    check(levels_per_call, resolution)
    return run(_steps(target, start, levels_per_call, resolution, cap, on_level, key="monthly_amount_today",
                      event="income_amount_search_iter", what="required-income"), probe_levels)
