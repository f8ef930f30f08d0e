"""Guardrail spending rules: a household that cuts back when it is drawing too fast and loosens up when it is drawing slowly.

The reference spends the same real amount every month of retirement whatever the portfolio does.  `SpendingRule` is a
withdrawal-rate guardrail in the style of Guyton-Klinger (``include/mcr.h``: ``mcr_spending_rule`` states the arithmetic): each
path carries a spending multiplier ``m`` (1 in retirement year 0) on its base expenses; at the start of every later retirement
year the path's real withdrawal rate relative to its initial one, ``q = m (B0 / P0) / (B / P)``, is compared with two
guardrails: ``q > upper`` cuts ``m`` by ``cut`` (never below ``floor``), ``q < lower`` raises it by ``raise_`` (never above
``ceiling``).  The path kernel runs the rule (``mcr_run_rule_rng``); `SpendingRuleOutcomes` holds what a count-only launch
returns about it: per retirement year, how many paths are still alive, how many spend less than they began with, how many
stand at the floor and how many spend more.  Pure integer and float arithmetic on those tables: no device.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _native as N

FIELDS = ("upper", "lower", "cut", "raise_", "floor", "ceiling")


@dataclass(frozen=True)
class SpendingRule:
    """The six values of ``mcr_spending_rule`` (``raise_`` is its ``raise``), validated by the library
    (``mcr_validate_spending_rule``; host only): ``upper >= 1``, ``0 <= lower <= 1``, ``0 <= cut < 1``, ``raise_ >= 0``,
    ``0 <= floor <= 1 <= ceiling``, all finite.  ``ValueError`` names the offending field."""

    upper: float
    lower: float
    cut: float
    raise_: float
    floor: float
    ceiling: float

    def __post_init__(self):
        for f in FIELDS:
            object.__setattr__(self, f, float(getattr(self, f)))
        rec = self.record()
        if N.load_library().mcr_validate_spending_rule(C.byref(rec)) != 0:
            raise ValueError(N.last_error() or "invalid spending rule")

    @classmethod
    def neutral(cls) -> "SpendingRule":
        """The rule that never moves ``m``: every result equals the fixed-spending one."""
        return cls(1.0, 1.0, 0.0, 0.0, 1.0, 1.0)

    @classmethod
    def parse(cls, text: str) -> "SpendingRule":
        """``"upper,lower,cut,raise,floor,ceiling"`` (the command line's form)."""
        parts = [p.strip() for p in str(text).split(",")]
        if len(parts) != 6:
            raise ValueError(f"a spending rule is six numbers upper,lower,cut,raise,floor,ceiling; got {text!r}")
        return cls(*[float(p) for p in parts])

    @property
    def is_neutral(self) -> bool:
        return self.cut == 0.0 and self.raise_ == 0.0

    def record(self) -> N.McrSpendingRule:
        r = N.McrSpendingRule()
        r.upper, r.lower, r.cut, r.floor, r.ceiling = self.upper, self.lower, self.cut, self.floor, self.ceiling
        setattr(r, "raise", self.raise_)
        return r

    def as_dict(self) -> Dict[str, float]:
        return {"upper": self.upper, "lower": self.lower, "cut": self.cut, "raise": self.raise_, "floor": self.floor,
                "ceiling": self.ceiling}


RULE_OPTION_AMOUNTS = ("initial_balance", "monthly_contribution", "monthly_expenses")


def rule_options(params_model, options: Sequence[dict]) -> List[tuple]:
    """The records of a rule probe (``engine.probe_rules``): ``(initial_balance, monthly_contribution, monthly_expenses, rule)``
    per mapping of ``options``.  ``"rule"`` is a `SpendingRule`, six numbers in its field order, or None / missing: the neutral
    rule, i.e. fixed spending (None in the record).  A missing amount takes the value of ``params_model`` (the config), an
    unknown key raises ``ValueError``; so does a rule outside its ranges, naming ``options[k].rule`` and the field."""
    defaults = tuple(float(getattr(params_model, f)) for f in RULE_OPTION_AMOUNTS)
    records = []
    for k, o in enumerate(options):
        unknown = sorted(set(o) - set(RULE_OPTION_AMOUNTS) - {"rule"})
        if unknown:
            raise ValueError(f"options[{k}]: unknown key(s) {unknown}; a rule option may set {['rule', *RULE_OPTION_AMOUNTS]}")
        rule = o.get("rule")
        if rule is not None and not isinstance(rule, SpendingRule):
            try:
                rule = SpendingRule(*[float(x) for x in rule])
            except (TypeError, ValueError) as exc:
                raise ValueError(f"options[{k}].rule: {exc}") from None
        records.append(tuple(float(o.get(f, d)) for f, d in zip(RULE_OPTION_AMOUNTS, defaults)) + (rule,))
    return records


class SpendingRuleOutcomes:
    """What one launch under a rule counts over ``n_paths`` paths.

    ``successes``: paths that succeed.  ``year_counts``: ``[retirement_years, 4]`` = per retirement year, over the paths that
    begin it alive and after its decision, ``{alive, cut (m < 1), at the floor (m <= floor < 1), raised (m > 1)}``
    (``mcr_rule_outputs.year_counts``).  ``retirement_age``: ``current_age + working_months / 12``.  ``ever_cut``: the number of
    paths whose multiplier was below 1 in any year, known only when the multiplier rows were requested (None otherwise)."""

    def __init__(self, successes: int, n_paths: int, year_counts, retirement_age: float, ever_cut: Optional[int] = None):
        self.successes = int(successes)
        self.n_paths = int(n_paths)
        self.year_counts = np.asarray(year_counts, dtype=np.int64)
        if self.year_counts.ndim != 2 or self.year_counts.shape[1] != N.MCR_RULE_N_COUNTS or self.year_counts.shape[0] < 1:
            raise ValueError(f"year_counts must be [retirement_years, {N.MCR_RULE_N_COUNTS}], got shape {self.year_counts.shape}")
        alive = self.year_counts[:, N.MCR_RULE_ALIVE]
        if self.successes < 0 or self.successes > self.n_paths or np.any(self.year_counts < 0) or np.any(alive > self.n_paths):
            raise ValueError("counts must be >= 0 and at most n_paths")
        if np.any(self.year_counts[:, 1:].max(axis=1) > alive) or np.any(self.year_counts[:, N.MCR_RULE_FLOOR] > self.year_counts[:, N.MCR_RULE_CUT]):
            raise ValueError("a year's cut / floor / raised paths are among its alive paths, and its floor paths among the cut ones")
        self.retirement_age = float(retirement_age)
        self.ever_cut = None if ever_cut is None else int(ever_cut)

    def __eq__(self, other) -> bool:
        if not isinstance(other, SpendingRuleOutcomes):
            return NotImplemented
        return (self.successes == other.successes and self.n_paths == other.n_paths and self.retirement_age == other.retirement_age
                and self.ever_cut == other.ever_cut and np.array_equal(self.year_counts, other.year_counts))

    __hash__ = None

    @property
    def retirement_years(self) -> int:
        return int(self.year_counts.shape[0])

    @property
    def probability(self) -> float:
        """Success %: count / n_paths * 100 in fp64, as the plain probes' callers compute it."""
        return float(np.float64(self.successes) / np.float64(self.n_paths) * 100.0)

    def _share(self, column: int) -> np.ndarray:
        return self.year_counts[:, column].astype(np.float64) / np.float64(self.n_paths)

    @property
    def alive_share(self) -> np.ndarray:
        """``[retirement_years]``: the share of ALL paths that begin each retirement year."""
        return self._share(N.MCR_RULE_ALIVE)

    @property
    def cut_share(self) -> np.ndarray:
        """... that begin it spending less than they started with."""
        return self._share(N.MCR_RULE_CUT)

    @property
    def floor_share(self) -> np.ndarray:
        """... that begin it at the rule's floor."""
        return self._share(N.MCR_RULE_FLOOR)

    @property
    def raised_share(self) -> np.ndarray:
        """... that begin it spending more than they started with."""
        return self._share(N.MCR_RULE_RAISED)

    @property
    def ages(self) -> np.ndarray:
        """The age at which each retirement year begins."""
        return self.retirement_age + np.arange(self.retirement_years, dtype=np.float64)

    @property
    def ever_cut_share(self) -> float:
        """The share of all paths that ever spent less than they started with; needs the multiplier rows."""
        if self.ever_cut is None:
            raise ValueError("ever_cut_share needs the multiplier rows (spending_rule_outcomes(..., multipliers=True))")
        return float(np.float64(self.ever_cut) / np.float64(self.n_paths))

    def years(self) -> List[Dict[str, float]]:
        a, c, f, r = self.alive_share, self.cut_share, self.floor_share, self.raised_share
        return [{"year": y, "age": float(self.ages[y]), "alive": float(a[y]), "cut": float(c[y]), "at_floor": float(f[y]),
                 "raised": float(r[y])} for y in range(self.retirement_years)]

    def row(self) -> Dict[str, object]:
        """The rule's part of a response document."""
        doc: Dict[str, object] = {"probability": self.probability, "n_paths": self.n_paths, "years": self.years()}
        if self.ever_cut is not None:
            doc["ever_cut_share"] = self.ever_cut_share
        return doc


SPENDING_QUANTILES = (0.05, 0.25, 0.50, 0.75, 0.95)


class SpendingBands:
    """The spending fan chart of a launch under a rule: per retirement year the 5 / 25 / 50 / 75 / 95 % REAL monthly spending
    ``monthly_expenses * m`` among the paths that begin the year alive, from ``multiplier_bins`` ``[retirement_years,
    n_m_bins + 2]`` binned on ``m_edges`` (``mcr_run_rule_year_bins_rng``).  ``estimate`` is the rank-interpolated value and
    ``lo`` / ``hi`` the bracket that contains the exact quantile (`aggregation.bands_from_bins`), each ``[retirement_years,
    5]``, scaled by the base ``monthly_expenses``; a year nobody begins is NaN, and a side outside the edges is infinite."""

    def __init__(self, multiplier_bins, m_edges, monthly_expenses: float, quantiles: Sequence[float] = SPENDING_QUANTILES):
        from . import aggregation as A

        self.multiplier_bins = np.asarray(multiplier_bins)
        self.m_edges = np.asarray(m_edges, dtype=np.float64)
        if self.multiplier_bins.ndim != 2 or self.multiplier_bins.shape[1] != self.m_edges.shape[0] + 1:
            raise ValueError(f"multiplier_bins must be [retirement_years, n_m_bins + 2] for {self.m_edges.shape[0]} edges, "
                             f"got shape {self.multiplier_bins.shape}")
        self.monthly_expenses = float(monthly_expenses)
        if not (np.isfinite(self.monthly_expenses) and self.monthly_expenses >= 0.0):
            raise ValueError("monthly_expenses must be finite and >= 0")
        self.quantiles = tuple(float(q) for q in quantiles)
        lo, hi, est = A.bands_from_bins(self.multiplier_bins, self.m_edges, list(self.quantiles))
        self.multiplier_lo, self.multiplier_hi, self.multiplier_estimate = lo, hi, est
        self.lo, self.hi, self.estimate = lo * self.monthly_expenses, hi * self.monthly_expenses, est * self.monthly_expenses
        self.alive = self.multiplier_bins.sum(axis=1).astype(np.int64)

    @property
    def retirement_years(self) -> int:
        return int(self.multiplier_bins.shape[0])

    def years(self) -> List[Dict[str, object]]:
        """Per year: ``alive`` paths and ``{"p50": {"estimate", "lo", "hi"}, ...}``; non-finite values are None."""
        def num(v):
            return float(v) if np.isfinite(v) else None
        out = []
        for y in range(self.retirement_years):
            row: Dict[str, object] = {"year": y, "alive": int(self.alive[y])}
            for j, q in enumerate(self.quantiles):
                row[f"p{int(round(q * 100))}"] = {"estimate": num(self.estimate[y, j]), "lo": num(self.lo[y, j]), "hi": num(self.hi[y, j])}
            out.append(row)
        return out
