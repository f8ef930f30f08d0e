"""The every-start replay of a recorded market: one path per month of the record the plan could have started in.

A ``"cohorts"`` history (``history.MarketHistory(..., scheme="cohorts")``) draws nothing: path ``i`` starts at month
``i mod H`` of an ``H``-month record and runs it forward, wrapping to the record's beginning when it runs off its end
(``include/mcr.h``: MCR_HISTORY_COHORTS).  ``RetirementMonteCarloSimulator.historical_cohorts`` runs exactly the ``H`` paths
``0 .. H - 1`` and hands their per-path summary to `CohortReplay`, which answers the backtest's questions from it: which
starts failed, which were the worst, and what the share of successes is over the starts whose horizon fits inside the record.
Pure NumPy on small arrays: no device.
"""

from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

from .history import month_label


class CohortReplay:
    """One cohort per start row ``0 .. H - 1`` of the record.

    ``success`` ``[H]`` bool, ``final_balance`` ``[H]``, ``years_to_ruin`` ``[H]`` (NaN where the cohort succeeds): the
    path kernel's per-path summary of path ``i`` = start row ``i``.  ``total_months``: the months a path lives (working +
    retirement).  ``first_month``: the ``"YYYY-MM"`` label of row 0, or ``None``.

    ``wraps[i] = i + total_months > H``: cohort ``i`` ran off the record's end and continued at its beginning — months that
    never followed one another in the record."""

    def __init__(self, success, final_balance, years_to_ruin, total_months: int, first_month: Optional[str] = None):
        self.success = np.asarray(success).astype(bool).reshape(-1)
        h = int(self.success.shape[0])
        if h < 1:
            raise ValueError("success: a replay has at least one cohort")
        self.final_balance = np.asarray(final_balance, dtype=np.float64).reshape(-1)
        self.years_to_ruin = np.asarray(years_to_ruin, dtype=np.float64).reshape(-1)
        if self.final_balance.shape[0] != h or self.years_to_ruin.shape[0] != h:
            raise ValueError(f"final_balance / years_to_ruin: {self.final_balance.shape[0]} / {self.years_to_ruin.shape[0]} entries for {h} cohorts")
        if int(total_months) < 0:
            raise ValueError(f"total_months: {total_months!r} is negative")
        self.total_months = int(total_months)
        self.first_month = first_month
        self.start_row = np.arange(h, dtype=np.int64)
        self.wraps = self.start_row + self.total_months > h
        self.start_month: List[Optional[str]] = [month_label(first_month, i) if first_month is not None else None for i in range(h)]

    def __len__(self) -> int:
        return int(self.success.shape[0])

    @staticmethod
    def _share(flags: np.ndarray) -> float:
        return float(np.float64(int(np.count_nonzero(flags))) / np.float64(int(flags.shape[0])) * 100.0)

    @property
    def success_probability(self) -> float:
        """Success % over all cohorts: count / H * 100 in fp64, as the simulator computes a batch's."""
        return self._share(self.success)

    @property
    def success_probability_complete(self) -> Optional[float]:
        """Success % over the cohorts that do not wrap; ``None`` when every cohort wraps (a record shorter than the horizon)."""
        keep = ~self.wraps
        return self._share(self.success[keep]) if np.any(keep) else None

    def worst(self, k: int) -> List[int]:
        """Start rows of the ``k`` worst cohorts: the failing ones that ran out soonest first, then the successful ones with
        the least left; ties by start row."""
        ruin = np.where(self.success, np.inf, np.nan_to_num(self.years_to_ruin, nan=np.inf))
        left = np.where(self.success, self.final_balance, 0.0)
        order = np.lexsort((self.start_row, left, ruin, self.success))     # (the last key sorts first: failures before successes)
        return [int(i) for i in order[:max(int(k), 0)]]

    def cohort(self, i: int) -> Dict[str, object]:
        i = int(i)
        ytr = float(self.years_to_ruin[i])
        return {"start_row": i, "start_month": self.start_month[i], "wraps": bool(self.wraps[i]), "success": bool(self.success[i]),
                "final_balance": float(self.final_balance[i]), "years_to_ruin": None if np.isnan(ytr) else ytr}

    def to_document(self, worst: int = 10) -> Dict[str, object]:
        """For JSON: the two probabilities, the counts, the ``worst`` worst cohorts in full and every cohort's columns."""
        return {
            "cohorts": len(self),
            "total_months": self.total_months,
            "first_month": self.first_month,
            "complete_cohorts": int(np.count_nonzero(~self.wraps)),
            "success_probability": self.success_probability,
            "success_probability_complete": self.success_probability_complete,
            "worst": [self.cohort(i) for i in self.worst(worst)],
            "start_month": list(self.start_month) if self.first_month is not None else None,
            "wraps": [bool(x) for x in self.wraps],
            "success": [bool(x) for x in self.success],
            "final_balance": [float(x) for x in self.final_balance],
            "years_to_ruin": [None if np.isnan(x) else float(x) for x in self.years_to_ruin],
        }


__all__ = ("CohortReplay",)
