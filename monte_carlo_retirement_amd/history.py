"""A recorded market as the engine's third random stream: paths resampled in blocks from a record.

The engine's own streams ask every question of one market model: three lognormal series with one correlation.  A
:class:`MarketHistory` asks it of sequences like the ones that occurred: monthly (equity, inflation, premium) shocks read
from a record in blocks of ``block_months`` consecutive months, each block starting at a uniformly drawn month and wrapping
around the record's end (``include/mcr.h``: ``MCR_RNG_HISTORY`` states the rule).  Inside a block the record's fat tails,
its volatility clustering and the co-movement of its series are kept as they were.

``scheme`` chooses the resampling rule (``include/mcr.h`` states all three as integer recipes):

* ``"block"`` (the default): every block ``block_months`` long;
* ``"stationary"``: the stationary bootstrap of Politis & Romano — block lengths geometric with MEAN ``block_months``, so
  no month of a path is a seam in every path and the resampled series is stationary;
* ``"cohorts"``: no resampling at all — path ``i`` starts at month ``i mod months`` of the record and runs it forward, the
  historical backtest itself ("would this plan have survived retiring into 1929?").  ``block_months`` is not used.  A
  success probability over ``n`` paths is the share over the starts ``0 .. n - 1 mod months``: ``n`` should be a multiple
  of the record's length, or some starts count once more than others
  (``RetirementMonteCarloSimulator.historical_cohorts`` runs exactly one path per start and says which start did what).

The table holds STANDARD shocks ``z`` — what ``exp(mu_log / 12 + sigma_log / sqrt(12) z)`` turns into a month's growth
factor — so one record has two readings:

* **the record's shape around the config's means** (the default): the config's own return, inflation and premium
  assumptions, with the record's sequence of surprises;
* **the record as it was**: ``with_fitted_market(config, history)`` replaces those assumptions by the record's own fitted
  ones, and the growth factors are the recorded ones again (to rounding).

``equity_inflation_correlation`` is not applied to a history: the record carries its own co-movement.

Pure Python / NumPy: nothing here touches the GPU.
"""

from __future__ import annotations

import csv
import math
import re
from typing import Dict, Optional, Sequence

import numpy as np

from .config import Config

MAX_HISTORY_MONTHS = 2048      # include/mcr.h: MCR_MAX_HISTORY_MONTHS
MAX_BLOCK_MONTHS = 2**31 - 1
_SERIES = ("inv1", "inflation", "inv2_premium")
SCHEMES = ("block", "stationary", "cohorts")      # include/mcr.h: MCR_HISTORY_BLOCK / _STATIONARY / _COHORTS, in this order


def month_label(first_month: str, offset: int) -> str:
    """``"YYYY-MM"`` of the month ``offset`` months after ``first_month``."""
    year, month = int(first_month[:4]), int(first_month[5:7])
    t = year * 12 + (month - 1) + int(offset)
    return f"{t // 12:04d}-{t % 12 + 1:02d}"


def _log_to_arithmetic(mu_log: float, sigma_log: float):
    """Inverse of ``params.arithmetic_to_log_params``: lognormal (mu, sigma) -> arithmetic annual (mean, volatility)."""
    one_plus_mean = math.exp(mu_log + 0.5 * sigma_log * sigma_log)
    return one_plus_mean - 1.0, one_plus_mean * math.sqrt(math.expm1(sigma_log * sigma_log))


class MarketHistory:
    """``z``: the table ``[months, 3]`` of standard shocks (equity, inflation, premium over inflation), 1..2048 months,
    finite.  ``block_months``: the block length of the bootstrap (1 = i.i.d. months; at least the horizon = one start per
    path, the record run forward from it).  ``fitted``: the annual log parameters the table was standardised with
    (``{"inv1" | "inflation" | "inv2_premium": (mu_log, sigma_log)}``) and the sample correlation, when it was built from
    returns; a table given directly has none.  ``scheme``: ``"block"``, ``"stationary"`` (``block_months`` is then the MEAN
    block length) or ``"cohorts"`` (``block_months`` is not used), see the module's text.  ``first_month``: an optional
    ``"YYYY-MM"`` label of row 0, used only to label cohorts."""

    def __init__(self, z, block_months: int = 12, fitted: Optional[Dict[str, object]] = None, *, scheme: str = "block",
                 first_month: Optional[str] = None):
        arr = np.array(z, dtype=np.float64, order="C")
        if arr.ndim != 2 or arr.shape[1] != 3:
            raise ValueError(f"z: shape {arr.shape} is not (months, 3)")
        if not 1 <= arr.shape[0] <= MAX_HISTORY_MONTHS:
            raise ValueError(f"z: {arr.shape[0]} months, the record must have 1..{MAX_HISTORY_MONTHS}")
        if not np.all(np.isfinite(arr)):
            raise ValueError("z: every entry must be finite")
        if isinstance(block_months, bool) or int(block_months) != block_months or not 1 <= int(block_months) <= MAX_BLOCK_MONTHS:
            raise ValueError(f"block_months: {block_months!r} is not an integer in 1..2^31 - 1")
        if not isinstance(scheme, str) or scheme not in SCHEMES:
            raise ValueError(f"scheme: {scheme!r} is not one of {', '.join(repr(s) for s in SCHEMES)}")
        if first_month is not None and (not isinstance(first_month, str) or not re.fullmatch(r"\d{4}-(0[1-9]|1[0-2])", first_month)):
            raise ValueError(f"first_month: {first_month!r} is not a 'YYYY-MM' month")
        arr.setflags(write=False)
        self.z = arr
        self.block_months = int(block_months)
        self.fitted = dict(fitted) if fitted is not None else None
        self.scheme = scheme
        self.first_month = first_month

    @property
    def months(self) -> int:
        return int(self.z.shape[0])

    @classmethod
    def from_monthly_returns(cls, equity, inflation, inv2=None, premium=None, block_months: int = 12, *, scheme: str = "block",
                             first_month: Optional[str] = None) -> "MarketHistory":
        """From SIMPLE monthly returns (0.01 = +1 %): the equity series, the inflation series, and exactly one of ``inv2``
        (the second asset's nominal return; its premium gross is its gross over inflation's) or ``premium`` (already over
        inflation).  Per series: ``z = (ln g - m) / s`` with the sample mean and standard deviation (ddof = 0) of the log
        gross returns, fitted ``mu_log = 12 m`` and ``sigma_log = sqrt(12) s`` — the inverse of
        ``exp(mu_log / 12 + sigma_log / sqrt(12) z)``.  A constant series gives ``z = 0`` and ``sigma_log = 0``."""
        if (inv2 is None) == (premium is None):
            raise ValueError("give exactly one of inv2 / premium")
        series = {"equity": equity, "inflation": inflation, ("inv2" if premium is None else "premium"): inv2 if premium is None else premium}
        gross = {}
        for name, values in series.items():
            r = np.asarray(values, dtype=np.float64)
            if r.ndim != 1:
                raise ValueError(f"{name}: shape {r.shape} is not one-dimensional")
            if not np.all(np.isfinite(r)):
                raise ValueError(f"{name}: every return must be finite")
            if np.any(1.0 + r <= 0.0):
                raise ValueError(f"{name}: a gross return 1 + r must be positive")
            gross[name] = 1.0 + r
        n = gross["equity"].shape[0]
        for name, g in gross.items():
            if g.shape[0] != n:
                raise ValueError(f"{name}: {g.shape[0]} months, equity has {n}")
        if not 1 <= n <= MAX_HISTORY_MONTHS:
            raise ValueError(f"equity: {n} months, the record must have 1..{MAX_HISTORY_MONTHS}")
        logs = [np.log(gross["equity"]), np.log(gross["inflation"]),
                np.log(gross["inv2"] / gross["inflation"]) if premium is None else np.log(gross["premium"])]
        z = np.zeros((n, 3), dtype=np.float64)
        fitted: Dict[str, object] = {}
        for c, (key, lg) in enumerate(zip(_SERIES, logs)):
            m, s = float(np.mean(lg)), float(np.std(lg))
            if np.all(lg == lg[0]):
                m, s = float(lg[0]), 0.0
            if s > 0.0:
                z[:, c] = (lg - m) / s
            fitted[key] = (12.0 * m, math.sqrt(12.0) * s)
        moving = fitted["inv1"][1] > 0.0 and fitted["inflation"][1] > 0.0      # (a constant series correlates with nothing)
        fitted["equity_inflation_correlation"] = float(np.corrcoef(logs[0], logs[1])[0, 1]) if moving else 0.0
        return cls(z, block_months, fitted, scheme=scheme, first_month=first_month)

    @classmethod
    def from_csv(cls, path: str, equity: str = "equity", inflation: str = "inflation", inv2: Optional[str] = "inv2",
                 premium: Optional[str] = None, block_months: int = 12, *, scheme: str = "block",
                 first_month: Optional[str] = None) -> "MarketHistory":
        """From a CSV file with a header line and one row per month, oldest first; the arguments name its columns of simple
        monthly returns.  Give ``premium`` (and ``inv2=None``) when the file holds the premium over inflation."""
        if (inv2 is None) == (premium is None):
            raise ValueError("give exactly one of inv2 / premium")
        want = {"equity": equity, "inflation": inflation, ("inv2" if premium is None else "premium"): inv2 if premium is None else premium}
        cols: Dict[str, list] = {k: [] for k in want}
        with open(path, "r", encoding="utf-8", newline="") as fh:
            reader = csv.DictReader(fh)
            for k, name in want.items():
                if reader.fieldnames is None or name not in reader.fieldnames:
                    raise ValueError(f"{k}: no column {name!r} in {path} (columns: {reader.fieldnames})")
            for line, row in enumerate(reader, start=2):
                for k, name in want.items():
                    try:
                        cols[k].append(float(row[name]))
                    except (TypeError, ValueError):
                        raise ValueError(f"{k}: column {name!r}, line {line} of {path}: {row[name]!r} is not a number") from None
        return cls.from_monthly_returns(cols["equity"], cols["inflation"], inv2=cols.get("inv2"), premium=cols.get("premium"),
                                        block_months=block_months, scheme=scheme, first_month=first_month)

    def fitted_assumptions(self) -> Dict[str, float]:
        """The ``Config`` fields that replay the record as it was: arithmetic annual means and volatilities (the inverse of
        ``params.arithmetic_to_log_params`` at the fitted log parameters), and the record's sample correlation of equity
        and inflation log returns — information only, a history launch does not apply it."""
        if self.fitted is None:
            raise ValueError("fitted: this history was given as a table of shocks; build it with from_monthly_returns / from_csv")
        m1, v1 = _log_to_arithmetic(*self.fitted["inv1"])
        mi, vi = _log_to_arithmetic(*self.fitted["inflation"])
        mp, vp = _log_to_arithmetic(*self.fitted["inv2_premium"])
        return {
            "inv1_returns_mean": m1, "inv1_returns_volatility": v1,
            "inflation_rate_mean": mi, "inflation_rate_volatility": vi,
            "inv2_premium_over_inflation_mean": mp, "inv2_premium_over_inflation_volatility": vp,
            "equity_inflation_correlation": float(self.fitted["equity_inflation_correlation"]),
        }


def with_fitted_market(config: Config, history: MarketHistory) -> Config:
    """``config`` with the record's own market in place of its assumptions: simulated with ``history``, the months' growth
    factors are the recorded ones."""
    return config.model_copy(update=history.fitted_assumptions(), deep=True)


def market_document(history: MarketHistory, as_recorded: bool) -> Dict[str, object]:
    """What a response document says about the history it was computed with (``examples/run_scenario.py``: key ``market``).
    ``scheme`` appears for the schemes other than ``"block"``, ``first_month`` when it was given."""
    doc: Dict[str, object] = {"months": history.months, "block_months": history.block_months, "as_recorded": bool(as_recorded)}
    if history.scheme != "block":
        doc["scheme"] = history.scheme
    if history.first_month is not None:
        doc["first_month"] = history.first_month
    if history.fitted is not None:
        doc["fitted"] = history.fitted_assumptions()
    return doc


def as_history(value) -> MarketHistory:
    if not isinstance(value, MarketHistory):
        raise ValueError("market_history must be a MarketHistory")
    return value


__all__: Sequence[str] = ("MarketHistory", "with_fitted_market", "market_document", "MAX_HISTORY_MONTHS", "SCHEMES")
