"""Paired comparison of options evaluated over the SAME random paths.

A joint probe (`engine.probe_*_joint`) returns, next to each option's success count, the option x option co-occurrence
matrix: ``joint[a][b]`` = paths on which options a and b both succeed.  Because the options share every path's random
numbers, most paths succeed or fail under both, and the difference between two success probabilities is decided by the
few DISCORDANT paths alone.  `JointOutcomes` turns the matrix into pair tables, the paired difference with its standard
error, the exact McNemar test and rescue shares.  Pure NumPy and `math`: no device.
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np


def mcnemar_p_value(n10: int, n01: int) -> float:
    """Exact two-sided McNemar p-value of ``n10`` against ``n01`` discordant paths: ``min(1, 2 P[X <= min(n10, n01)])`` for
    ``X ~ Binomial(n10 + n01, 1/2)``; 1.0 without discordant paths.  The tail is summed in log space (`math.lgamma`), from
    its largest term down, so a million discordant paths neither overflow nor underflow to 0."""
    n10, n01 = int(n10), int(n01)
    if n10 < 0 or n01 < 0:
        raise ValueError(f"discordant counts must be >= 0, got {n10}, {n01}")
    m, k = n10 + n01, min(n10, n01)
    if m == 0:
        return 1.0
    log_half_m = -m * math.log(2.0)
    lg_m1 = math.lgamma(m + 1.0)

    def log_term(i: int) -> float:
        return lg_m1 - math.lgamma(i + 1.0) - math.lgamma(m - i + 1.0) + log_half_m

    # terms i = k, k - 1, ... decrease (k <= m / 2): sum them relative to the largest until they no longer register
    top = log_term(k)
    total = 0.0
    for i in range(k, -1, -1):
        t = math.exp(log_term(i) - top)
        total += t
        if t < 1e-17 * total:
            break
    log_p = math.log(2.0) + top + math.log(total)
    return 1.0 if log_p >= 0.0 else max(math.exp(log_p), 5e-324)


class JointOutcomes:
    """The joint outcomes of ``n`` options over ``n_paths`` shared paths.

    ``joint``: ``[n, n]`` integers, ``joint[a][b]`` = paths on which a and b both succeed (the diagonal is each option's
    success count).  ``extremes``: ``(paths on which every option succeeds, paths on which none does)`` or None."""

    def __init__(self, joint, n_paths: int, extremes=None):
        j = np.asarray(joint, dtype=np.int64)
        if j.ndim != 2 or j.shape[0] != j.shape[1]:
            raise ValueError(f"joint must be a square matrix, got shape {j.shape}")
        self.joint = j
        self.n_paths = int(n_paths)
        self.extremes = None if extremes is None else (int(extremes[0]), int(extremes[1]))

    def __len__(self) -> int:
        return int(self.joint.shape[0])

    @property
    def successes(self) -> np.ndarray:
        return self.joint.diagonal().copy()

    @property
    def probabilities(self) -> np.ndarray:
        """Success % per option: count / n_paths * 100 in fp64, as the plain probes' callers compute it."""
        return np.array([float(np.float64(int(c)) / np.float64(self.n_paths) * 100.0) for c in self.joint.diagonal()],
                        dtype=np.float64)

    @property
    def all_succeed(self) -> Optional[int]:
        return None if self.extremes is None else self.extremes[0]

    @property
    def none_succeed(self) -> Optional[int]:
        return None if self.extremes is None else self.extremes[1]

    def pair(self, a: int, b: int) -> Dict[str, int]:
        """The 2 x 2 table of options a and b over the shared paths."""
        j = self.joint
        n11 = int(j[a][b])
        n10 = int(j[a][a]) - n11
        n01 = int(j[b][b]) - n11
        return {"both": n11, "only_a": n10, "only_b": n01, "neither": self.n_paths - n11 - n10 - n01}

    def difference(self, a: int, b: int) -> Dict[str, Optional[float]]:
        """Option a against option b.  ``delta`` = P(a) - P(b) in points; ``se`` its paired standard error, from the
        discordant paths; ``se_unpaired`` what two independent batches would give; ``p_value`` the exact two-sided McNemar
        test of "a and b succeed equally often"; ``rescued`` the share of a's failures on which b succeeds (None when a
        never fails)."""
        t = self.pair(a, b)
        n10, n01, big_n = t["only_a"], t["only_b"], self.n_paths
        fails_a = big_n - int(self.joint[a][a])
        pa, pb = int(self.joint[a][a]) / big_n, int(self.joint[b][b]) / big_n
        return {
            "delta": 100.0 * (n10 - n01) / big_n,
            "se": 100.0 * math.sqrt(max((n10 + n01) - (n10 - n01) ** 2 / big_n, 0.0)) / big_n,
            "se_unpaired": 100.0 * math.sqrt(pa * (1.0 - pa) / big_n + pb * (1.0 - pb) / big_n),
            "p_value": mcnemar_p_value(n10, n01),
            "rescued": None if fails_a == 0 else n01 / fails_a,
        }

    def indistinguishable_from(self, a: int, alpha: float = 0.05) -> List[int]:
        """The options the paired test cannot tell from a at level `alpha` (a itself included)."""
        return [b for b in range(len(self)) if b == a or self.difference(a, b)["p_value"] >= alpha]
