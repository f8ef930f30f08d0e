"""Per-option outcomes of options evaluated over the SAME random paths: when a plan fails, and what a plan that works leaves.

An outcomes probe (`engine.probe_*_outcomes`) returns, next to each option's success count, two rows per option: the final
balance of the paths that succeed and the YearsToRuin of the paths that fail.  `engine.ruin_month_counts` reduces the ruin
rows to one count per month of the horizon and `aggregation.row_quantiles` gives the quantiles of the successful cohort's
final balance.  `OptionOutcomes` holds those small tables and answers from them: "with 95 % confidence the money lasts to
age 91", the median age of ruin among the paths that fail, the 5th to 95th percentile of what is left.  Pure integer and
float arithmetic on the tables: no device.

Month ``m`` of a ruin table is ``rint(12 * YearsToRuin)``: 0 = the plan fails before retirement (a tax bill it cannot pay),
``m`` in ``1 .. 12 ry`` = it fails in the m-th month of retirement (or, at ``12 ry``, at the terminal settlement).
"""

from __future__ import annotations

from fractions import Fraction
from typing import Dict, Optional, Sequence

import numpy as np

DEFAULT_QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)
CONFIDENCE_LEVELS = (0.90, 0.95, 0.99)    # the "lasts_until_age" keys of the claim and stress tables: "90", "95", "99"


def quantile_key(q: float) -> str:
    """``0.05 -> "p5"``, ``0.5 -> "p50"``, ``0.975 -> "p97.5"``."""
    return f"p{float(q) * 100.0:.10g}"


class OptionOutcomes:
    """The outcomes of ``k`` options over ``n_paths`` shared paths.

    ``successes``: ``[k]`` success counts.  ``ruin_months``: ``[k, 12 * retirement_years + 1]`` paths ruined per month.
    ``quantiles`` / ``final_quantiles``: the requested quantiles and their values ``[k, len(quantiles)]`` over the final
    balances of each option's successful paths (ignored where ``cohort[k] == 0``); ``cohort``: ``[k]`` sizes of those cohorts.
    ``retirement_age``: ``current_age + working_months / 12``."""

    def __init__(self, successes, n_paths: int, ruin_months, quantiles: Sequence[float], final_quantiles, cohort, retirement_age: float):
        self.successes = np.asarray(successes, dtype=np.int64).reshape(-1)
        self.n_paths = int(n_paths)
        k = int(self.successes.shape[0])
        self.ruin_months = np.asarray(ruin_months, dtype=np.int64)
        if self.ruin_months.ndim != 2 or self.ruin_months.shape[0] != k or self.ruin_months.shape[1] < 13 or (self.ruin_months.shape[1] - 1) % 12 != 0:
            raise ValueError(f"ruin_months must be [{k}, 12 * retirement_years + 1], got shape {self.ruin_months.shape}")
        self.quantiles = tuple(float(q) for q in quantiles)
        self.final_quantiles = np.asarray(final_quantiles, dtype=np.float64).reshape(k, len(self.quantiles))
        self.cohort = np.asarray(cohort, dtype=np.int64).reshape(-1)
        if self.cohort.shape[0] != k:
            raise ValueError(f"{k} options but {self.cohort.shape[0]} cohort sizes")
        if np.any(self.successes < 0) or np.any(self.ruin_months < 0) or np.any(self.successes + self.ruin_months.sum(axis=1) > self.n_paths):
            raise ValueError("successes and ruined paths must be >= 0 and sum to at most n_paths per option")
        self.retirement_age = float(retirement_age)

    def __len__(self) -> int:
        return int(self.successes.shape[0])

    def __eq__(self, other) -> bool:
        if not isinstance(other, OptionOutcomes):
            return NotImplemented
        return (self.n_paths == other.n_paths and self.quantiles == other.quantiles and self.retirement_age == other.retirement_age
                and np.array_equal(self.successes, other.successes) and np.array_equal(self.ruin_months, other.ruin_months)
                and np.array_equal(self.cohort, other.cohort)
                and np.array_equal(self.final_quantiles, other.final_quantiles, equal_nan=True))

    __hash__ = None

    @property
    def horizon_months(self) -> int:
        return int(self.ruin_months.shape[1]) - 1

    @property
    def probabilities(self) -> np.ndarray:
        """Success % per option: count / n_paths * 100 in fp64, as the plain probes' callers compute it."""
        return np.array([float(np.float64(int(c)) / np.float64(self.n_paths) * 100.0) for c in self.successes], dtype=np.float64)

    def failures(self, k: int) -> int:
        return int(self.ruin_months[k].sum())

    def ruined_by(self, k: int) -> np.ndarray:
        """``[12 ry + 1]``: the share of ALL paths ruined in months ``<= m`` under option k."""
        return np.cumsum(self.ruin_months[k]).astype(np.float64) / np.float64(self.n_paths)

    def lasts_months(self, k: int, confidence: float) -> Optional[int]:
        """The largest month ``m`` such that the share of paths ruined in months ``<= m`` is ``<= 1 - confidence``: with that
        confidence the money is still there after month m.  None when that holds through the whole horizon (the plan does
        not fail that often at all); -1 when it fails even month 0 (more than ``1 - confidence`` of the paths fail before
        retirement).  The comparison is exact: `confidence` is read as the decimal it is written as (0.95 = 19/20) and
        compared with integer path counts, so a confidence that sits exactly on a step of the curve includes that step."""
        c = Fraction(repr(float(confidence)))
        if not (0 < c <= 1):
            raise ValueError(f"confidence {confidence} must be in (0, 1]")
        allowed = (1 - c) * self.n_paths
        cum = np.cumsum(self.ruin_months[k])
        if int(cum[-1]) <= allowed:
            return None
        # cum is non-decreasing: the first month above the allowance ends the run
        return int(np.searchsorted(cum, int(allowed // 1), side="right")) - 1

    def lasts_until_age(self, k: int, confidence: float) -> Optional[float]:
        """`lasts_months` as an age: ``retirement_age + m / 12`` (the retirement age itself where the plan fails that
        confidence before retirement); None when the money lasts the whole horizon with that confidence."""
        m = self.lasts_months(k, confidence)
        return None if m is None else self.retirement_age + max(m, 0) / 12.0

    def median_ruin_age(self, k: int) -> Optional[float]:
        """The median age at ruin among the paths that fail under option k (the mean of the two middle paths for an even
        count, as `pandas.Series.median`); None without failures."""
        f = self.failures(k)
        if f == 0:
            return None
        cum = np.cumsum(self.ruin_months[k])
        lo = int(np.searchsorted(cum, (f - 1) // 2, side="right"))     # month of the failure of 0-based rank (f - 1) // 2
        hi = int(np.searchsorted(cum, f // 2, side="right"))
        return self.retirement_age + (lo + hi) / 2.0 / 12.0

    def final_balance(self, k: int) -> Dict[float, Optional[float]]:
        """``{quantile: nominal final balance}`` of the paths that succeed under option k; every value None for an empty
        cohort."""
        if int(self.cohort[k]) == 0:
            return {q: None for q in self.quantiles}
        return {q: float(v) for q, v in zip(self.quantiles, self.final_quantiles[k])}

    def row(self, k: int) -> Dict[str, object]:
        """The keys `compare_claiming_options` and `stress_test` add to row k with ``outcomes=True``."""
        return {
            "lasts_until_age": {f"{round(c * 100):d}": self.lasts_until_age(k, c) for c in CONFIDENCE_LEVELS},
            "median_ruin_age": self.median_ruin_age(k),
            "final_balance": {quantile_key(q): v for q, v in self.final_balance(k).items()},
        }
