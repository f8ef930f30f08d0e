"""Drop-in host surface of the engine: ``RetirementMonteCarloSimulator``.

Same class name, constructor, attributes, method names, argument meaning, return shapes and
error behaviour as the reference's simulator (rflamino/monte_carlo_retirement,
backend/simulation.py:126-1342) so FastAPI / CLI / search callers and the reference's own
tests work unchanged — but every path is simulated by the hand-written HIP kernels in csrc/
(through the C ABI of include/mcr.h).  There is no CPU fallback: without a gfx950 device the
compute methods raise ``RuntimeError``.

What differs, by design (documented in DESIGN.md):
* random numbers come from a counter-based Philox4x32-10 + Box-Muller stream keyed by
  ``main_seed`` with counter (path index, month, stream id) instead of NumPy
  SeedSequence -> PCG64 -> ziggurat; ``path_seed`` therefore means *global path index*;
  common random numbers across working-month candidates hold exactly as in the reference;
* the pandas aggregation (quantile bands, counts) is computed on the device with the same
  arithmetic (NumPy ``linear`` interpolation, NaN skipping).
"""

from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd

from . import _native as N
from . import aggregation as A
from . import distributed as D
from . import engine as E
from ._logging import logger
from .config import Config
from .constants import MONTHS_PER_YEAR, SMALL_EPSILON
from .params import arithmetic_to_log_params, params_from_config

__all__ = [
    "RetirementMonteCarloSimulator",
    "arithmetic_to_log_params",
    "retirement_age",
    "stream_payment_start_age",
    "stream_payment_start_month_index",
    "age_at_retirement_year",
    "years_from_t0_to_age",
    "median_first_year_withdrawal_rate",
    "trajectory_time_points",
]

SUMMARY_COLUMNS = [  # simulation.py:1013-1024 (column order of summary_df)
    "Start Balance",
    "Final Balance",
    "Success",
    "YearsToRuin",
    "First Year Gross Withdrawal",
    "First Year Real Gross Withdrawal",
    "Inflation At Retirement",
]
_FIELD_OF = {
    "Start Balance": "start_balance",
    "Final Balance": "final_balance",
    "YearsToRuin": "years_to_ruin",
    "First Year Gross Withdrawal": "first_year_gross_withdrawal",
    "First Year Real Gross Withdrawal": "first_year_real_gross_withdrawal",
    "Inflation At Retirement": "inflation_at_retirement",
}


# ---- module-level helpers (simulation.py:32-123) ----------------------------------------------
def retirement_age(current_age: float, working_months: int) -> float:
    """Age when retirement starts (simulation.py:32-34)."""
    return current_age + working_months / MONTHS_PER_YEAR


def stream_payment_start_age(current_age: float, working_months: int, start_at_age: float) -> float:
    """Payments start once eligible AND retired (simulation.py:37-44)."""
    return max(retirement_age(current_age, working_months), float(start_at_age))


def stream_payment_start_month_index(current_age: float, working_months: int, start_at_age: float) -> int:
    """First retirement-month index paid (simulation.py:47-63): ceil of the gap in months, with the
    reference's 1e-6 guard so an exact month boundary does not round up."""
    gap_years = stream_payment_start_age(current_age, working_months, start_at_age) - retirement_age(
        current_age, working_months
    )
    return max(0, int(math.ceil(gap_years * MONTHS_PER_YEAR - SMALL_EPSILON)))


def age_at_retirement_year(current_age: float, working_months: int, year_num: int) -> float:
    """Age at the start of retirement year ``year_num`` (simulation.py:66-70)."""
    return retirement_age(current_age, working_months) + year_num


def years_from_t0_to_age(current_age: float, target_age: float) -> float:
    """Years from T=0 until ``target_age`` (simulation.py:73-75)."""
    return max(0.0, float(target_age) - float(current_age))


def median_first_year_withdrawal_rate(summary_df: pd.DataFrame) -> float:
    """Median over paths (start balance > eps) of first-year real gross withdrawal / start
    balance, in percent (simulation.py:78-96)."""
    if summary_df.empty:
        return float("nan")
    col = (
        "First Year Real Gross Withdrawal"
        if "First Year Real Gross Withdrawal" in summary_df.columns
        else "First Year Gross Withdrawal"
    )
    start = summary_df["Start Balance"]
    keep = start > SMALL_EPSILON
    if not keep.any():
        return float("nan")
    return float(((summary_df[col][keep] / start[keep]) * 100.0).median())


def trajectory_time_points(working_months: int, retirement_years: int) -> List[float]:
    """Year values of the yearly trajectory samples (simulation.py:99-123)."""
    full_years, leftover = divmod(working_months, MONTHS_PER_YEAR)
    t_ret = working_months / MONTHS_PER_YEAR
    pts = [0.0] + [float(y) for y in range(1, full_years + 1)]
    if leftover:
        pts.append(t_ret)
    pts.extend(t_ret + y for y in range(1, retirement_years + 1))
    return pts


def trajectory_sample_months(working_months: int, retirement_years: int) -> List[int]:
    """`trajectory_time_points` in whole months from today: the sample at ``m`` is the balance behind month ``m``."""
    wm = int(working_months)
    full_years, leftover = divmod(wm, MONTHS_PER_YEAR)
    pts = [MONTHS_PER_YEAR * y for y in range(full_years + 1)]
    if leftover:
        pts.append(wm)
    pts.extend(wm + MONTHS_PER_YEAR * y for y in range(1, int(retirement_years) + 1))
    return pts


def allocation_by_sample(glide_path, working_months: int, retirement_years: int) -> List[float]:
    """The weight of asset 1 the portfolio stands at in each yearly sample of `trajectory_time_points` under `glide_path` (an
    `allocation.GlidePath`): the weight in force during the month the sample closes, ``W[min((m - 1) // 12, n - 1)]`` for the
    sample behind month ``m`` (the month's rebalance brought the balance to it), and ``W[0]`` today.  Exact from the table."""
    return [float(glide_path.weight_at(max(0, m - 1))) for m in trajectory_sample_months(working_months, retirement_years)]


def _gather_columns(rows, picked) -> np.ndarray:
    """``rows[:, picked].T`` as a host array.  Each pick is a strided column VIEW (``select`` is metadata only: the
    64-bit offset is folded into the view's data pointer on the host) and the stack kernel then indexes k tensors of
    T elements each.  No torch INDEXING kernel (``index_select`` / advanced indexing) ever sees the [2T+ry, stride]
    slab, which exceeds 2**32 elements from ~3.2e7 paths on: the one GPU-side abort of round 1 was such a gather
    on a 3.3e7-path slab (LABNOTES.md, rounds 1-3 section 11)."""
    import torch

    return torch.stack([rows[:, int(g)] for g in picked]).cpu().numpy()


class _SummaryDownload:
    """summary_df (simulation.py:1012-1027) from a device batch, in two halves so that the transfer overlaps the device
    work that follows the path kernel.  `start`: the six float columns and the flags go device->host as plain contiguous 1-D
    copies into ONE pinned [6, n] buffer (no stack / indexing kernel on the device, so the element count any torch kernel sees
    stays n whatever the batch size) on a COPY STREAM of its own that waits for the path kernel only — 56 bytes a path: 560 MB
    at 10^7 paths, tens of milliseconds of PCIe time that used to sit, serially, between the path kernel and the band
    selection (round 3: 131 ms end to end for 77 ms of kernels).  `frame`: waits for the copy stream and wraps the buffer in a
    no-copy DataFrame with the reference's column order and dtypes."""

    def __init__(self, batch, n: int):
        torch = batch.torch
        dev = batch.success.device
        self.fields = list(_FIELD_OF.items())
        main = torch.cuda.current_stream(dev)
        self.stream = _copy_stream(torch, dev)
        # (the pinned buffers come from torch's caching host allocator: allocated while the path kernel runs)
        self.host = torch.empty((len(self.fields), n), dtype=torch.float64, pin_memory=True)
        self.flags = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        self.stream.wait_stream(main)                    # = after the path kernel that was just enqueued
        with torch.cuda.stream(self.stream):
            for i, (_, f) in enumerate(self.fields):
                self.host[i].copy_(batch.summary[f][:n], non_blocking=True)
            self.flags.copy_(batch.success[:n], non_blocking=True)
        self._batch = batch                               # the source tensors stay alive until the copies have run

    def frame(self) -> pd.DataFrame:
        self.stream.synchronize()
        self._batch = None
        h = self.host.numpy()
        cols = {name: h[i] for i, (name, _) in enumerate(self.fields)}
        cols["Success"] = self.flags.numpy().view(np.bool_)
        return pd.DataFrame({c: cols[c] for c in SUMMARY_COLUMNS}, copy=False)


_copy_streams: Dict[Tuple[int, int], object] = {}


def _copy_stream(torch, dev):
    """One side stream per (thread, device) for device->host transfers that overlap kernels on the caller's stream."""
    import threading

    key = (threading.get_ident(), dev.index or 0)
    st = _copy_streams.get(key)
    if st is None:
        st = _copy_streams[key] = torch.cuda.Stream(device=dev)
    return st


def _summary_frame(batch, n: int) -> pd.DataFrame:
    """The whole download in one call (callers with nothing to overlap it with)."""
    return _SummaryDownload(batch, n).frame()


class _BackgroundCall:
    """`fn(*args)` on a host thread of its own; `result()` joins and returns its value or re-raises its exception."""

    def __init__(self, fn, *args):
        import threading

        self._value, self._error = None, None

        def run():
            try:
                self._value = fn(*args)
            except BaseException as exc:  # noqa: BLE001  (handed to the caller's thread)
                self._error = exc

        self._thread = threading.Thread(target=run, daemon=True)
        self._thread.start()

    def result(self):
        self._thread.join()
        if self._error is not None:
            raise self._error
        return self._value


def sample_columns(seed: int, n: int, k: int):
    """``numpy.random.RandomState(seed).choice(n, k, replace=False)`` — the column indices pandas' ``DataFrame.sample(n=k,
    axis=1, random_state=seed)`` picks (simulation.py:1063-1078) — or None (error logged) where NumPy raises, as the
    reference does (:1079-1083; e.g. seed >= 2**32).  NumPy shuffles all n indices for it; the library's restatement
    (``mcr_sample_columns``: same MT19937 draws, the k positions traced back through the swaps) returns the same indices in
    about half the time — it has to hide under a kernel launch of n paths."""
    if 0 <= int(seed) < 2**32 and 1 <= k <= 64 and k <= n <= 2**32:
        out = np.empty(k, dtype=np.int64)
        rc = N.load_library().mcr_sample_columns(int(seed), int(n), int(k), out.ctypes.data)
        if rc == 0:
            return out
    try:
        return np.random.RandomState(seed).choice(int(n), size=int(k), replace=False)
    except ValueError as ve:
        logger.error(f"Error sampling trajectories: {ve}")
        return None


def _fold_seed_u64(seed: int) -> int:
    """Philox key = the seed folded to 64 bits (seeds are unbounded Python ints in the Config)."""
    s, out = int(seed), 0
    while True:
        out ^= s & 0xFFFFFFFFFFFFFFFF
        s >>= 64
        if s == 0:
            return out


class RetirementMonteCarloSimulator:
    """Monte Carlo retirement simulator whose paths run on an MI355X (see module docstring)."""

    def __init__(self, params_model: Config, main_seed_override: Optional[int] = None, device: int = 0,
                 rng: str = "philox", market_history=None):
        """``rng="philox"`` (default): the engine's counter-based stream; ``path_seed`` = global path
        index.  ``rng="numpy"``: the reference's OWN stream reproduced on the device (SeedSequence ->
        PCG64 -> ziggurat): the same ``seed`` then yields the reference's numbers, ``path_seed`` is the
        reference's uint32 path seed and `_path_seeds` follows its spawn-and-cache rule (:187-199).
        ``rng="history"`` with ``market_history`` = a :class:`history.MarketHistory`: months resampled in
        blocks from a recorded market (``include/mcr.h``: MCR_RNG_HISTORY); ``path_seed`` = global path
        index, the block starts are keyed by the seed, and ``equity_inflation_correlation`` is NOT applied
        (the record carries its own co-movement).  The record's shocks run around the config's own means
        and volatilities; ``history.with_fitted_market(config, h)`` gives the config that replays the
        record as it was.  Probes run one launch per level on this stream.  The history's ``scheme`` chooses
        the rule: fixed blocks, the stationary bootstrap, or ``"cohorts"`` — path i starts at month
        i mod H of the H-month record, so a success probability over n paths is the share over the
        starts 0 .. n - 1 mod H and n should be a multiple of H (`historical_cohorts` runs exactly H)."""
        if rng not in ("philox", "numpy", "history"):
            raise ValueError("rng must be 'philox', 'numpy' or 'history'")
        if rng == "history" and market_history is None:
            raise ValueError("rng='history' needs market_history (a MarketHistory)")
        if rng != "history" and market_history is not None:
            raise ValueError(f"market_history is given but rng is {rng!r}: pass rng='history'")
        self.rng = rng
        self.params_model = params_model.model_copy(deep=True)  # simulation.py:136

        if main_seed_override is not None:  # :138-145
            if main_seed_override < 0:
                raise ValueError("main_seed_override must be nonnegative.")
            self.main_seed = main_seed_override
        elif self.params_model.seed is not None:
            self.main_seed = self.params_model.seed
        else:
            # No seed configured: the reference hashes the current time (utils.py:16-18).  With one process per
            # GPU every rank would draw its OWN seed — different Philox keys per shard, different sampled
            # columns per rank — so rank 0's seed is broadcast and every rank uses it.
            self.main_seed = D.broadcast_int(_seed_from_timestamp()) if D.is_active() else _seed_from_timestamp()

        # Two independent streams (search vs final run, :147-151): the stream id is one word of the
        # Philox counter, so the streams never overlap.
        self._stream_name = "final"
        self._engine_seed = _fold_seed_u64(self.main_seed)
        self.market_history = None
        self._history_rng = None
        if rng == "history":
            from .history import SCHEMES, MarketHistory, as_history

            h = as_history(market_history)
            if D.is_active():     # every rank must resample the same record by the same rule: rank 0's, like its seed
                h = MarketHistory(D.broadcast_array(h.z), D.broadcast_int(h.block_months), h.fitted,
                                  scheme=SCHEMES[D.broadcast_int(SCHEMES.index(h.scheme))], first_month=h.first_month)
            self.market_history = h
            self._history_rng = N.history_rng(self._engine_seed, h.z, h.block_months, SCHEMES.index(h.scheme))   # (owns its copy of the table)
        self.device = int(device)
        #: under torch.distributed, batches smaller than this are computed in full on EVERY rank (identical
        #: results, no communication): a 50 000-path probe is latency-bound (~1 ms) and sharding it would add
        #: an all-reduce + host sync per probe.  Larger batches are sharded across the ranks.
        self.shard_min_paths = 1_000_000
        #: under torch.distributed, sharded batches of MORE paths than this deliver the per-path summary frame (n x 7: 56 bytes
        #: a path, 5.6 GB at 1e8 paths) to rank 0 ONLY — the other ranks get a frame with the reference's columns and no rows —
        #: instead of all-gathering it into the host memory of every rank.  Everything else of the 7-tuple (bands, sampled
        #: paths, observation counts) is identical on all ranks either way; `results.compact_result` needs no per-path frame.
        self.gather_all_max_paths = 20_000_000
        #: which ranks hold the rows of the last sharded run's `summary_df`: "all", or "rank0" (a deliberate empty frame elsewhere)
        self.last_summary_scope = "all"
        # NumPy stream bookkeeping: children spawned so far per stream, and the offset at which each
        # (stream, n) batch was spawned — the reference's _path_seed_cache rule (:154, :192-199)
        self._np_children_spawned = {"search": 0, "final": 0}
        self._np_batch_offset: Dict[Tuple[str, int], int] = {}

        p = self.params_model
        self._inv1_mu_log, self._inv1_sigma_log = arithmetic_to_log_params(  # :157-166
            p.inv1_returns_mean, p.inv1_returns_volatility
        )
        self._inf_mu_log, self._inf_sigma_log = arithmetic_to_log_params(
            p.inflation_rate_mean, p.inflation_rate_volatility
        )
        self._inv2_prem_mu_log, self._inv2_prem_sigma_log = arithmetic_to_log_params(
            p.inv2_premium_over_inflation_mean, p.inv2_premium_over_inflation_volatility
        )
        self._equity_inflation_rho = p.equity_inflation_correlation  # :170
        self._params = params_from_config(p)
        logger.info(
            f"Simulator initialized for scenario '{p.Nickname}' with main seed: {self.main_seed}"
        )

    # ---- seed streams (:177-199) ---------------------------------------------------------------
    @property
    def _stream_id(self) -> int:
        return N.MCR_STREAM_SEARCH if self._stream_name == "search" else N.MCR_STREAM_FINAL

    def use_search_seeds(self) -> None:
        self._stream_name = "search"

    def use_final_seeds(self) -> None:
        self._stream_name = "final"

    def _path_seeds(self, num_simulations: int) -> List[int]:
        """Path identifiers of a batch.  Philox stream: a path's "seed" is its global index in the
        active stream.  NumPy stream: the reference's uint32 seeds, spawned once per (stream, n) and
        cached (:187-199).  Either way the list is the same for every working-month candidate."""
        n = int(num_simulations)
        if self.rng != "numpy":
            return list(range(n))
        off = self._np_offset(n)  # children (stream, off .. off+n-1) of SeedSequence(main_seed)
        return [
            int(np.random.SeedSequence(self.main_seed, spawn_key=(self._stream_id, off + j)).generate_state(1)[0])
            for j in range(n)
        ]

    def _local_device(self) -> int:
        """The GPU this process computes on: the configured device, or — with one process per GPU under
        torch.distributed — the rank's current device."""
        if D.is_active():
            import torch

            return int(torch.cuda.current_device())
        return self.device

    def _np_offset(self, n: int) -> int:
        """Spawn offset of the (active stream, n) batch: assigned on first use, then cached."""
        key = (self._stream_name, int(n))
        if key not in self._np_batch_offset:
            self._np_batch_offset[key] = self._np_children_spawned[self._stream_name]
            self._np_children_spawned[self._stream_name] += int(n)
        return self._np_batch_offset[key]

    def _batch_rng(self, n: int):
        """RNG descriptor of an n-path batch on the active stream (int = Philox key)."""
        if self.rng == "philox":
            return self._engine_seed
        if self.rng == "history":
            return self._history_rng
        return N.numpy_rng(self.main_seed, child_offset=self._np_offset(n))

    # ---- scalar helpers: evaluated by the SAME device functions the path kernel inlines -----------
    def _calculate_withdrawal_and_update(
        self, bal_inv: float, cb_inv: float, net_withdrawal_target_for_inv: float,
        use_real_tax: bool, real_tax_rate: float,
    ) -> Tuple[float, float, float, float]:
        """(new_balance, new_cost_basis, gross_withdrawal, net_cash) — simulation.py:201-254."""
        r = E.eval_helper_host(
            N.MCR_HELPER_WITHDRAW, None,
            [[bal_inv, cb_inv, net_withdrawal_target_for_inv, 1.0 if use_real_tax else 0.0, real_tax_rate]],
            self._local_device(),
        )[0]
        return float(r[0]), float(r[1]), float(r[2]), float(r[3])

    def _net_liquidation_value(
        self, balance: float, cost_basis: float, use_realized_gains_tax: bool, realized_gains_tax_rate: float
    ) -> float:
        """Cash after liquidating an asset and paying gains tax — simulation.py:256-272."""
        return float(E.eval_helper_host(
            N.MCR_HELPER_NLV, None,
            [[balance, cost_basis, 1.0 if use_realized_gains_tax else 0.0, realized_gains_tax_rate]],
            self._local_device(),
        )[0][0])

    def _rebalance_portfolio(
        self, bal_inv1: float, cb_inv1: float, bal_inv2: float, cb_inv2: float
    ) -> Tuple[float, float, float, float]:
        """Tax-aware rebalance to the target allocation — simulation.py:274-359."""
        r = E.eval_helper_host(N.MCR_HELPER_REBALANCE, self._current_params(),
                               [[bal_inv1, cb_inv1, bal_inv2, cb_inv2]], self._local_device())[0]
        return float(r[0]), float(r[1]), float(r[2]), float(r[3])

    def _apply_annual_gain_taxes(
        self, balance_inv1: float, cost_basis_inv1: float, balance_inv2: float, cost_basis_inv2: float,
        gain_inv1: float, gain_inv2: float,
    ) -> Tuple[float, float, float, float, bool]:
        """Annual mark-to-market tax for one period — simulation.py:361-450."""
        r = E.eval_helper_host(
            N.MCR_HELPER_ANNUAL_TAX, self._current_params(),
            [[balance_inv1, cost_basis_inv1, balance_inv2, cost_basis_inv2, gain_inv1, gain_inv2]],
            self._local_device(),
        )[0]
        return float(r[0]), float(r[1]), float(r[2]), float(r[3]), bool(r[4])

    def _monthly_gross_from_shock(self, mu_log: float, sigma_log: float, z: float) -> float:
        """exp(mu/12 + sigma/sqrt(12) z) — simulation.py:468-474."""
        return float(E.eval_helper_host(N.MCR_HELPER_MONTHLY_GROSS, None, [[mu_log, sigma_log, z]], self._local_device())[0][0])

    def _draw_shock_path(self, n_months: int, path_seed: int) -> np.ndarray:
        """Shock rows (equity, inflation, premium) of one path, shape (n_months, 3) — the engine's
        replacement of simulation.py:452-466."""
        if self.rng == "numpy":
            return E.draw_shocks_host(
                N.numpy_rng(self.main_seed), self._stream_id, 0, 1, int(n_months), self._equity_inflation_rho,
                self._local_device(), path_seeds=np.array([int(path_seed)], dtype=np.uint32),
            )[0]
        return E.draw_shocks_host(
            self._batch_rng(1), self._stream_id, int(path_seed), 1, int(n_months), self._equity_inflation_rho,
            self._local_device(),
        )[0]

    def _current_params(self):
        """The parameter block of the *current* params_model (validate_assignment lets callers
        mutate the config between runs, as they can in the reference)."""
        self._params = params_from_config(self.params_model)
        return self._params

    # ---- one path (:476-950) -------------------------------------------------------------------
    def _run_single_simulation_path(
        self, working_months: int, path_seed: int
    ) -> Dict[str, Union[float, List[float]]]:
        """Simulate ONE path on the device and return the reference's 10-key dict."""
        if self.rng == "numpy":
            r = E.run_batch_host(
                self._current_params(), N.numpy_rng(self.main_seed), self._stream_id, 0, 1,
                int(working_months), want_bins=False, device=self._local_device(),
                path_seeds=np.array([int(path_seed)], dtype=np.uint32),
            )
        else:
            r = E.run_batch_host(
                self._current_params(), self._batch_rng(1), self._stream_id, int(path_seed), 1,
                int(working_months), want_bins=False, device=self._local_device(),
            )
        return {
            "Start Balance": float(r["start_balance"][0]),
            "Final Balance": float(r["final_balance"][0]),
            "Success": bool(r["success"][0]),
            "YearsToRuin": float(r["years_to_ruin"][0]),
            "First Year Gross Withdrawal": float(r["first_year_gross_withdrawal"][0]),
            "First Year Real Gross Withdrawal": float(r["first_year_real_gross_withdrawal"][0]),
            "Trajectory": r["trajectory"][:, 0].tolist(),
            "RealTrajectory": r["real_trajectory"][:, 0].tolist(),
            "WithdrawalRateTrajectory": r["withdrawal_rate_trajectory"][:, 0].tolist(),
            "Inflation At Retirement": float(r["inflation_at_retirement"][0]),
        }

    # ---- the historical backtest: one path per start month of the record ------------------------
    def historical_cohorts(self, working_months: int):
        """On a ``"cohorts"`` history of H months: ONE summary launch of exactly the H paths 0 .. H - 1 of the
        final stream — cohort i lives its first month in month i of the record — as a :class:`cohorts.CohortReplay`
        (per start: success, final balance, YearsToRuin, whether it wrapped around the record's end)."""
        from .cohorts import CohortReplay

        h = self.market_history
        if h is None or h.scheme != "cohorts":
            raise ValueError("historical_cohorts needs rng='history' with a market_history of scheme='cohorts'")
        wm = int(working_months)
        params = self._current_params()
        r = E.run_batch_host(params, self._history_rng, N.MCR_STREAM_FINAL, 0, h.months, wm, want_trajectories=False,
                             want_bins=False, device=self._local_device())
        return CohortReplay(r["success"], r["final_balance"], r["years_to_ruin"], int(E.query_sizes(params, wm).total_months), h.first_month)

    # ---- batch driver (:952-1128) --------------------------------------------------------------
    def run_monte_carlo_simulations(
        self, working_months: int, num_simulations: int
    ) -> Tuple[
        pd.DataFrame,
        Optional[pd.DataFrame],
        Optional[List[List[float]]],
        Optional[pd.DataFrame],
        Optional[pd.DataFrame],
        Optional[List[List[float]]],
        Optional[List[int]],
    ]:
        """Simulate ``num_simulations`` paths in ONE kernel launch and aggregate on the device.

        Returns the reference's 7-tuple: ``(summary_df, trajectory_percentiles_df,
        sample_trajectories, wr_percentiles_df, real_trajectory_percentiles_df,
        sample_real_trajectories, wr_observation_counts)``.
        """
        n = int(num_simulations)
        wm = int(working_months)
        if D.is_active() and n >= self.shard_min_paths:
            return self._run_sharded(wm, n)
        dev = self._local_device()
        logger.debug(f"Running {n} simulations on HIP device {dev} for {wm} working months.")
        batch = E.DeviceBatch(self._current_params(), wm, n, want="full", device=dev)
        batch.launch(self._batch_rng(n), self._stream_id, 0)
        # The 5 sampled columns are the ones trajectory_df.sample(n=5, axis=1, random_state=main_seed) picks (:1063-1078):
        # pandas draws them with RandomState(seed).choice(n, 5, replace=False), which permutes all n indices — 7 ms at 1e6
        # paths, as long as the kernel itself.  It is host-only work: done HERE, while the (asynchronous) launch runs.
        # (at 10^7 paths the draw is 30-50 ms of sequential host work — as long as the path kernel: it runs on a host thread of
        #  its own (the library call releases the GIL) and is joined where the sampled columns are gathered)
        sampler = _BackgroundCall(self._sample_columns, n) if n >= 200_000 else None
        picked = None if sampler else self._sample_columns(n)
        # Device -> host of the per-path summary (56 B / path) on the copy stream, behind the path kernel only; the band
        # selection (K3) is enqueued on the main stream right after and runs while the summary crosses the host link; the
        # frame is built last (the reference builds it first, simulation.py:1012-1027: same values, another order of work)
        download = _SummaryDownload(batch, n)

        traj_q, real_q, wr_q, wr_counts = A.band_quantiles(batch, n)
        qcols = pd.Index(list(A.TRAJECTORY_QUANTILES), dtype="float64")
        trajectory_percentiles_df = pd.DataFrame(traj_q, columns=qcols)
        real_trajectory_percentiles_df = pd.DataFrame(real_q, columns=qcols)
        wr_percentiles_df = pd.DataFrame(wr_q, columns=pd.Index(list(A.WR_QUANTILES), dtype="float64"))
        wr_observation_counts = [int(v) for v in wr_counts.tolist()]

        sample_trajectories_list: Optional[List[List[float]]] = None
        sample_real_trajectories_list: Optional[List[List[float]]] = None
        if sampler:
            picked = sampler.result()
        if picked is not None:
            sample_trajectories_list = _gather_columns(batch.trajectory, picked).tolist()
            sample_real_trajectories_list = _gather_columns(batch.real_trajectory, picked).tolist()
        summary_df = download.frame()
        return (
            summary_df,
            trajectory_percentiles_df,
            sample_trajectories_list,
            wr_percentiles_df,
            real_trajectory_percentiles_df,
            sample_real_trajectories_list,
            wr_observation_counts,
        )

    def _sample_columns(self, n: int):
        """Indices of the sampled paths — ``RandomState(main_seed).choice(n, min(n, 5), replace=False)``, what pandas'
        ``sample(n=5, axis=1, random_state=main_seed)`` draws (:1063-1078) — or None where the reference logs an error and
        returns no samples (e.g. main_seed >= 2**32, :1079-1083).  The same on every rank of a process group."""
        k = min(int(n), 5)
        if k <= 0:
            return None
        return sample_columns(self.main_seed, int(n), k)

    def _run_sharded(self, wm: int, n: int):
        """run_monte_carlo_simulations with one process per GPU (torch.distributed initialised): every rank
        simulates its shard of the global path range [0, n) and keeps its trajectories in its own HBM; the
        per-path summary is all-gathered (49 B/path; above `gather_all_max_paths` paths: gathered to rank 0 only,
        the reference's `summary_df` contract being a single-process one, simulation.py:1012-1027), the quantile bands come from the distributed radix
        select (digit histograms summed across ranks), the sampled paths are contributed by the rank that
        owns them.  Every rank returns the same bands, sampled paths and observation counts, bit-identical to the single-GPU
        result; `summary_df` is the single-GPU frame on every rank up to `gather_all_max_paths` paths and, above that, on rank 0
        ONLY — the other ranks then return a frame with the reference's columns and NO rows, and
        `self.last_summary_scope == "rank0"` tells such a caller that the empty frame is deliberate ("all" otherwise)."""
        import torch
        import torch.distributed as dist

        rank, world = dist.get_rank(), dist.get_world_size()
        dev = torch.cuda.current_device()
        begin, count = D.shard_range(n, rank, world)
        per = -(-n // world)
        batch = E.DeviceBatch(self._current_params(), wm, max(count, 1), want="full", device=dev)
        if count > 0:
            batch.launch(self._batch_rng(n), self._stream_id, begin, count)
        sampler = _BackgroundCall(self._sample_columns, n)   # (host work on a thread of its own; identical on every rank)
        comm = D._comm_device()
        # ---- per-path summary: pack [7, per] (six doubles + the flag), all-gather, trim ----
        fields = list(_FIELD_OF.values())
        local = torch.zeros((len(fields) + 1, per), dtype=torch.float64, device=batch.success.device)
        if count > 0:
            for i, f in enumerate(fields):
                local[i, :count] = batch.summary[f][:count]
            local[len(fields), :count] = batch.success[:count].to(torch.float64)
        local = local.to(comm)
        to_rank0_only = n > self.gather_all_max_paths
        self.last_summary_scope = "rank0" if to_rank0_only else "all"
        if to_rank0_only:
            logger.warning(f"{n} paths over {world} ranks: the per-path summary frame goes to rank 0 only "
                           f"(gather_all_max_paths = {self.gather_all_max_paths}); the other ranks return an empty frame")
            gathered = [torch.empty_like(local) for _ in range(world)] if rank == 0 else None
            pending = dist.gather(local, gathered, dst=0, async_op=True)
        else:
            gathered = [torch.empty_like(local) for _ in range(world)]
            pending = dist.all_gather(gathered, local, async_op=True)
        # ---- bands: enqueued while the summary gather is in flight (the selection's own small collectives queue behind it) ----
        traj_q, real_q, wr_q, wr_counts = D.sharded_band_quantiles(batch, count)
        pending.wait()
        del local
        if gathered is None:
            summary_df = pd.DataFrame({c: pd.Series(dtype=bool if c == "Success" else np.float64) for c in SUMMARY_COLUMNS})
        else:
            # trimmed and joined on the HOST (64-bit NumPy indexing whatever n is)
            allf = np.concatenate([g[:, :D.shard_range(n, r, world)[1]].cpu().numpy() for r, g in enumerate(gathered)], axis=1)
            del gathered
            cols = {name: allf[i] for i, name in enumerate(_FIELD_OF.keys())}
            cols["Success"] = allf[len(fields)] != 0.0
            summary_df = pd.DataFrame({c: cols[c] for c in SUMMARY_COLUMNS})
        qcols = pd.Index(list(A.TRAJECTORY_QUANTILES), dtype="float64")
        trajectory_percentiles_df = pd.DataFrame(traj_q, columns=qcols)
        real_trajectory_percentiles_df = pd.DataFrame(real_q, columns=qcols)
        wr_percentiles_df = pd.DataFrame(wr_q, columns=pd.Index(list(A.WR_QUANTILES), dtype="float64"))
        wr_observation_counts = [int(v) for v in wr_counts.tolist()]
        # ---- the 5 sampled paths: owner ranks fill their columns, the rest stays 0, sum-reduce ----
        samples = real_samples = None
        picked = sampler.result()
        if picked is not None:    # (None on every rank or on none: same seed, same n — the collective below cannot be skipped by one rank)
            T = batch.sizes.trajectory_len
            buf = torch.zeros((2, len(picked), T), dtype=torch.float64, device=batch.trajectory.device)
            for j, g in enumerate(picked):
                if begin <= g < begin + count:
                    buf[0, j] = batch.trajectory[:, g - begin]
                    buf[1, j] = batch.real_trajectory[:, g - begin]
            buf = buf.to(comm)
            D.all_reduce_sum_(buf)
            samples = buf[0].cpu().numpy().tolist()
            real_samples = buf[1].cpu().numpy().tolist()
        return (summary_df, trajectory_percentiles_df, samples, wr_percentiles_df,
                real_trajectory_percentiles_df, real_samples, wr_observation_counts)

    def _success_probability(self, summary_df: pd.DataFrame) -> float:
        """Share of paths that funded all spending, in percent (simulation.py:1130-1136)."""
        if summary_df.empty:
            return 0.0
        if "Success" in summary_df.columns:
            return float(summary_df["Success"].astype(bool).mean() * 100.0)
        return float((summary_df["Final Balance"] > SMALL_EPSILON).mean() * 100.0)

    # ---- count-only probes used by the search ------------------------------------------------------
    @staticmethod
    def _count_percent(count, n: int) -> float:
        """Success % from a probe's counter: the per-path route's ``mean() * 100`` bit for bit, count/n*100 in fp64."""
        return float(np.float64(int(count)) / np.float64(n) * 100.0)

    def _probe_many(self, months: Sequence[int], num_simulations: int) -> Dict[int, float]:
        """Success % of several candidate working-month counts over the same paths, from count-only
        kernels run concurrently (``mcr_probe_months_rng``).  Each value equals
        ``_success_probability(run_monte_carlo_simulations(m, n)[0])`` bit-for-bit: count/n*100.

        Under a process group: batches of at least ``shard_min_paths`` are sharded by path range (every
        rank counts all candidates on its shard); smaller ones are split by CANDIDATE (rank r takes
        ``months[r::world]`` over the whole range).  Either way the counter block is summed with one
        all-reduce and every rank sees the same probabilities (and replays the same search)."""
        months = [int(m) for m in months]
        n = int(num_simulations)
        params, rng, dev = self._current_params(), self._batch_rng(n), self._local_device()

        def probe(path_begin, count, ms):
            return E.probe_months(params, rng, self._stream_id, path_begin, count, ms, device=dev)

        counts = D.probe_candidates(months, n, self.shard_min_paths, probe)
        return {m: self._count_percent(counts[i, N.MCR_CTR_SUCCESS], n) for i, m in enumerate(months)}

    def _probe_success_probability(self, working_months: int, num_simulations: int) -> float:
        """Success % of one batch from the count-only kernel (no per-path HBM traffic)."""
        return self._probe_many([working_months], num_simulations)[int(working_months)]

    def _speculation_slots(self, num_simulations: int) -> int:
        """How many candidate months one round of the search may evaluate together at the cost of (about) one.
        Under a process group small batches are split by candidate across the ranks: every rank takes one candidate for
        free.  On ONE GPU a small probe is latency-bound — 50 000 paths are 782 wavefronts on 1 024 SIMDs — and candidates of
        one call share their accumulation sweep (`mcr_probe_months_rng`): measured at 50 000 paths, months 217+, one candidate
        1.19 ms, two 1.40, four 1.82 (tools/probe_latency.py).  Three candidates a round = the bisection's midpoint and both
        midpoints of the next level (two levels per round), or three bracket points: 1.6 ms instead of 2 x 1.19.  A month the
        reference would not have probed never reaches the curve or the callback (`ahead` in find_minimum_working_months).
        Large probes (>= 200 000 paths) fill the chip on their own: nothing is evaluated on speculation there."""
        if D.is_active() and int(num_simulations) < self.shard_min_paths:
            import torch.distributed as dist

            return dist.get_world_size()
        return 3 if int(num_simulations) < 200_000 else 1

    # ---- search driver (:1138-1342) ------------------------------------------------------------
    def find_minimum_working_months(
        self,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
    ) -> Tuple[int, float, List[Dict[str, float]]]:
        """Smallest working-month count reaching the target success probability.

        Same procedure as the reference: coarse bracket (step 12, grown to 24 while > 20 points
        short), bisection, then every month of the statistically plausible window is verified
        (3-sigma binomial margin) because Monte Carlo estimates are locally non-monotone.  Uses the
        search stream with common random numbers.  Returns ``(months, probability, search_curve)``;
        ``months == -1`` when the target is not reachable within 70 years.
        """
        # the reference's tests (and callers) may replace run_monte_carlo_simulations per instance;
        # then the search must go through it.  Otherwise use the count-only kernels.
        # (replaced on the instance, by a subclass, or by patching the class attribute)
        patched = ("run_monte_carlo_simulations" in self.__dict__
                   or getattr(type(self), "run_monte_carlo_simulations", None) is not _ENGINE_RUN)
        return self._search_minimum_working_months(self._probe_many, verbose, progress_callback, patched=patched)

    def find_minimum_working_months_with_rule(
        self,
        rule,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
    ) -> Tuple[int, float, List[Dict[str, float]]]:
        """`find_minimum_working_months` for a household that follows `rule` (a `spending_rules.SpendingRule`) once it has
        retired: how much sooner can I retire if I accept the guardrail?  The same driver, stream, path count, return shape
        and events; every round of candidates is ONE rule-grid probe with one level per row (``mcr_probe_rule_grid_rng``:
        the accumulation runs once for the round's months).  With `SpendingRule.neutral` the result, curve and events are
        exactly `find_minimum_working_months`'."""
        return self._search_minimum_working_months(lambda months, n: self._probe_many_with_rule(months, n, rule),
                                                   verbose, progress_callback)

    def _probe_many_with_rule(self, months: Sequence[int], num_simulations: int, rule) -> Dict[int, float]:
        """`_probe_many` under `rule`: success % of several candidate working-month counts over the same paths, at the
        config's own spending level, from one rule-grid probe with one level per row."""
        months = [int(m) for m in months]
        grid = self._rule_grid_probabilities(months, [[float(self.params_model.monthly_expenses)]] * len(months), rule,
                                             int(num_simulations))
        return {m: float(grid[i, 0]) for i, m in enumerate(months)}

    def _search_minimum_working_months(self, probe_many, verbose: bool, progress_callback, patched: bool = False
                                       ) -> Tuple[int, float, List[Dict[str, float]]]:
        """The driver of the month searches: bracket, bisection, verification window and the `ahead` speculation, over
        ``probe_many(months, n) -> {month: %}``.  ``patched``: go through `run_monte_carlo_simulations` month by month."""
        self.use_search_seeds()
        p = self.params_model
        first = p.starting_working_months_search
        target = p.target_probability
        n_sims = p.num_simulations_search
        horizon = first + 70 * MONTHS_PER_YEAR
        curve: List[Dict[str, float]] = []
        memo: Dict[int, float] = {}
        state = {"iter": 0, "best_seen": -1.0, "lo": first, "hi": None}
        # Unless `patched`, evaluate candidates the driver is about to ask for TOGETHER with the one
        # it asks for now (they share the GPU concurrently / are split across ranks).  `ahead` only
        # holds results early: months are still reported one by one, in the reference's order, and a
        # month the reference would not have probed never reaches memo, the curve or the callback.
        ahead: Dict[int, float] = {}
        slots = 1 if patched else self._speculation_slots(n_sims)

        if verbose:
            logger.info(f"Estimating working months to achieve {target:.2f}% success for '{p.Nickname}'.")
            logger.info(f"Starting search from {first} months. Simulations per test: {n_sims}.")

        def probe(months: int, likely_next: Sequence[int] = ()) -> float:
            if months in memo:
                return memo[months]
            state["iter"] += 1
            if verbose:
                logger.info(f"Search iter {state['iter']}: Testing {months} m "
                            f"({months / MONTHS_PER_YEAR:.1f} yrs) with {n_sims} sims.")
            if patched:
                summary_df = self.run_monte_carlo_simulations(months, n_sims)[0]
                prob = self._success_probability(summary_df)
            else:
                if months not in ahead:
                    batch = [months] + [m for m in dict.fromkeys(likely_next)
                                        if m != months and m not in ahead and m not in memo]
                    ahead.update(probe_many(batch, n_sims))
                prob = ahead[months]
            memo[months] = prob
            if verbose:
                logger.info(f"  Search iter {state['iter']}: Prob for {months} m: {prob:.2f}% (Target: {target:.2f}%)")
            years = round(months / MONTHS_PER_YEAR, 1)
            curve.append({"working_months": months, "working_years": years, "probability": round(prob, 2)})
            if progress_callback:
                progress_callback({
                    "type": "search_iter", "iteration": state["iter"], "working_months": months,
                    "working_years": years, "probability": round(prob, 2), "target": target,
                    "sim_count": n_sims, "lo": state["lo"], "hi": state["hi"],
                })
            state["best_seen"] = max(state["best_seen"], prob)
            return prob

        def bisection_mids(lo: int, hi: int, budget: int) -> List[int]:
            """Midpoints the bisection can reach from (lo, hi), breadth first, at most ``budget``."""
            out: List[int] = []
            frontier = [(lo, hi)]
            while frontier and len(out) < budget:
                nxt_frontier = []
                for a, b in frontier:
                    if b - a > 1 and len(out) < budget:
                        mid = (a + b) // 2
                        out.append(mid)
                        nxt_frontier += [(a, mid), (mid, b)]
                frontier = nxt_frontier
            return out

        # phase 1: bracket
        step = 12
        at = first
        prob_lo = probe(at)
        if prob_lo >= target:
            if verbose:
                logger.info(f"  Target met at starting point {at} months.")
            return at, prob_lo, curve
        best_prob = prob_lo
        while at < horizon:
            shortfall = target - prob_lo
            step = max(step, 24 if shortfall > 20 else (12 if shortfall > 10 else 6))
            nxt = min(at + step, horizon)
            if nxt <= at:
                break
            # the step never shrinks, so the following bracket points are (almost always) nxt + k*step
            prob = probe(nxt, [min(nxt + k * step, horizon) for k in range(1, slots)])
            if prob >= target:
                state["lo"], state["hi"], best_prob = at, nxt, prob
                if verbose:
                    logger.info(f"  Bracketed: lo={at} m (miss), hi={nxt} m (hit). Bisecting…")
                if progress_callback:
                    progress_callback({"type": "search_refining", "working_months": nxt, "lo": at, "hi": nxt})
                break
            state["lo"] = nxt
            prob_lo = prob
            at = nxt
        if state["hi"] is None:
            if verbose:
                logger.warning(f"Search for '{p.Nickname}' reached max limit "
                               f"({horizon / MONTHS_PER_YEAR:.1f} yrs). Target NOT met.")
                logger.warning(f"Highest probability achieved: {state['best_seen']:.2f}%.")
            return -1, state["best_seen"], curve

        # phase 2: bisect, remembering the smallest month that met the target
        best = state["hi"]
        while state["hi"] - state["lo"] > 1:
            mid = (state["lo"] + state["hi"]) // 2
            prob = probe(mid, bisection_mids(state["lo"], state["hi"], slots))
            if prob >= target:
                best, best_prob = mid, prob
                state["hi"] = mid
            else:
                state["lo"] = mid

        # phase 3: verify every month from one tested point before the first plausible month
        margin = min(100.0, 150.0 / math.sqrt(n_sims))
        tested = sorted(m for m in memo if m <= best)
        near = next((i for i, m in enumerate(tested) if memo[m] >= target - margin), len(tested) - 1)
        verify_from = max(first, tested[max(0, near - 1)])
        if verbose:
            logger.info(f"  Verifying each month from {verify_from} to {best} "
                        "to handle locally non-monotone Monte Carlo estimates.")
        window = list(range(verify_from, best + 1))
        for month in window:
            probe(month, window)   # every month of the window is needed: evaluate them in one batch
        hits = [m for m, pr in memo.items() if first <= m <= best and pr >= target]
        if hits:
            best = min(hits)
            best_prob = memo[best]
        if verbose:
            logger.info(f"  Search complete: estimated minimum {best} months "
                        f"({best / MONTHS_PER_YEAR:.1f} yrs) with prob {best_prob:.2f}%.")
        return best, best_prob, curve


    # ---- maximum-spending search -----------------------------------------------------------------
    def _level_probabilities(self, engine_probe, working_months: int, levels: Sequence, num_simulations: Optional[int],
                             lead: tuple = ()) -> np.ndarray:
        """The body of every `success_probability_by_*` whose probe returns counters alone: `engine_probe` is the `engine`
        function (`E.probe_expenses`, `E.probe_scenarios`, ...), ``levels`` its levels or records and ``lead`` the
        arguments it takes in front of them (the income probe's stream index)."""
        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        wm = int(working_months)
        params, rng, dev = self._current_params(), self._batch_rng(n), self._local_device()

        def probe(path_begin, count, idx):
            return engine_probe(params, rng, self._stream_id, path_begin, count, wm, *lead, [levels[i] for i in idx], device=dev)

        if not levels:
            return np.zeros(0, dtype=np.float64)
        counts = D.probe_candidates(list(range(len(levels))), n, self.shard_min_paths, probe)
        return np.array([self._count_percent(counts[i, N.MCR_CTR_SUCCESS], n) for i in range(len(levels))], dtype=np.float64)

    def _option_records(self, family: str, options: Sequence[dict], stream=None) -> Tuple[List[tuple], tuple]:
        """What is specific to an option family -- ``"scenarios"``, ``"income"``, ``"assumptions"``, ``"allocations"``, ``"glide_paths"`` or ``"rules"``, which is also
        the middle of its three `engine` entry points ``probe_<family>``, ``probe_<family>_joint`` and
        ``probe_<family>_outcomes``: ``(records, lead)``, the validated records of ``options`` and the arguments the engine
        calls take in front of them.  Raises ``ValueError`` as the family's record builder does."""
        p = self.params_model
        if family == "scenarios":
            from .nestegg import scenario_records

            return scenario_records(options, (p.initial_balance, p.monthly_contribution, p.monthly_expenses)), ()
        if family == "income":
            from .income import income_options, stream_index

            index = stream_index(p, stream)
            return income_options(p, index, options), (index,)
        if family == "assumptions":
            from .stress import assumption_records

            return assumption_records(p, options), ()
        if family == "allocations":
            from .allocation import allocation_records

            return allocation_records(p, options), ()
        if family == "glide_paths":     # (a record carries its own table: a shard of the options is a call of its own)
            from .allocation import glide_records

            records, table = glide_records(p, options)
            return [(*r[:3], tuple(table[r[3]:r[3] + r[4]])) for r in records], ()
        from .spending_rules import rule_options

        return rule_options(p, options), ()

    def _option_probabilities(self, family: str, working_months: int, options: Sequence[dict], num_simulations: Optional[int],
                              stream=None) -> np.ndarray:
        """The body of `success_probability_by_scenarios`, `..._by_income_options` and `..._by_assumptions`."""
        records, lead = self._option_records(family, options, stream)
        if not records:
            return np.zeros(0, dtype=np.float64)
        return self._level_probabilities(getattr(E, f"probe_{family}"), working_months, records, num_simulations, lead)

    def _option_probe(self, kind: str, family: str, working_months: int, options: Sequence[dict], num_simulations: Optional[int],
                      stream=None, quantiles=None):
        """The body of every `joint_outcomes_by_*` (``kind = "joint"``) and `option_outcomes_by_*` (``"outcomes"``): the
        family's records, validated before any device work, through ``engine.probe_<family>_<kind>`` (looked up at call time)
        into `_joint_outcomes` / `_option_outcomes`.  The rule probes also return their year counts, which are not asked for."""
        records, lead = self._option_records(family, options, stream)
        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        wm = int(working_months)
        params, rng, dev = self._current_params(), self._batch_rng(n), self._local_device()
        extra = dict({"masks": None} if kind == "joint" else {}, **({"year_counts": False} if family == "rules" else {}))

        def probe(path_begin, count):
            out = getattr(E, f"probe_{family}_{kind}")(params, rng, self._stream_id, path_begin, count, wm, *lead, records,
                                                       device=dev, **extra)
            return out[:1] + out[2:] if family == "rules" else out      # (counts, year counts, ...) -> (counts, ...)

        if kind == "joint":
            return self._joint_outcomes(probe, len(records), n)
        return self._option_outcomes(probe, len(records), wm, n, quantiles)

    def _joint_outcomes(self, joint_probe, n_records: int, num_simulations: Optional[int]):
        """The body of the `joint_outcomes_by_*` methods: ``joint_probe(path_begin, count) -> (counts, joint, extremes, masks)``
        is an `engine.probe_*_joint` call over ALL the records.  A pair table needs both options on the same path, so under
        a process group the batch is always sharded by PATH RANGE (never by option) and the ``n^2 + 2`` integers are summed
        in one all-reduce: every rank returns the same `paired.JointOutcomes`; masks stay on their rank."""
        import torch

        from .paired import JointOutcomes

        k = int(n_records)
        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        if k == 0:
            return JointOutcomes(np.zeros((0, 0), dtype=np.int64), n, (0, 0))

        def probe(path_begin, count, _):
            _, joint, extremes, _ = joint_probe(path_begin, count)
            return torch.cat([joint.reshape(-1), extremes.reshape(-1)])

        flat = D.probe_candidates([0], n, 0, probe, width=k * k + 2)[0]
        return JointOutcomes(flat[:k * k].reshape(k, k), n, (int(flat[k * k]), int(flat[k * k + 1])))

    def _option_outcomes(self, outcomes_probe, n_records: int, working_months: int, num_simulations: Optional[int], quantiles):
        """The body of the `option_outcomes_by_*` methods: ``outcomes_probe(path_begin, count) -> (counts, final_rows,
        ruin_rows)`` is an `engine.probe_*_outcomes` call over ALL the records.  Under a process group the batch is sharded
        by PATH RANGE as `_joint_outcomes` shards it: the success counts and the ruin-month counts (``k (12 ry + 2)``
        integers) are summed in one all-reduce, the final-balance quantiles of the successful cohorts come from the
        distributed radix select (`distributed.sharded_row_quantiles`); the rows stay on their rank and every rank returns
        the same `outcomes.OptionOutcomes`."""
        import torch

        from .outcomes import OptionOutcomes

        k = int(n_records)
        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        ry = int(self.params_model.retirement_years)
        cells = 12 * ry + 1
        qs = tuple(float(q) for q in quantiles)
        if any(not (0.0 <= q <= 1.0) for q in qs):
            raise ValueError(f"quantiles must lie in [0, 1], got {qs}")
        age = retirement_age(self.params_model.current_age, int(working_months))
        if k == 0:
            return OptionOutcomes(np.zeros(0, dtype=np.int64), n, np.zeros((0, cells), dtype=np.int64), qs,
                                  np.zeros((0, len(qs))), np.zeros(0, dtype=np.int64), age)
        local = {}

        def probe(path_begin, count, _):
            counts, final_rows, ruin_rows = outcomes_probe(path_begin, count)
            local["rows"], local["n"] = final_rows, int(count)
            months = E.ruin_month_counts(ruin_rows, count, ry)
            return torch.cat([counts[:, N.MCR_CTR_SUCCESS].reshape(-1), months.reshape(-1)])

        flat = D.probe_candidates([0], n, 0, probe, width=k + k * cells)[0]
        successes, months = flat[:k], flat[k:].reshape(k, cells)
        final_q, cohort = np.full((k, len(qs)), np.nan), successes.copy()
        if qs and n > 0:
            rows = local.get("rows")
            if rows is None or local["n"] == 0:      # (a rank whose shard of the path range is empty still takes part in the selection)
                dev = torch.device("cuda", self._local_device())
                rows, local["n"] = torch.full((k, 64), float("nan"), dtype=torch.float64, device=dev), 0
            final_q, cohort = D.sharded_row_quantiles(rows, local["n"], qs)
        return OptionOutcomes(successes, n, months, qs, final_q, cohort, age)

    def success_probability_by_expenses(self, working_months: int, monthly_expenses: Sequence[float],
                                        num_simulations: Optional[int] = None) -> np.ndarray:
        """Success % of each ``monthly_expenses`` level at ``working_months``, over the active seed stream's batch of
        ``num_simulations`` paths (default ``num_simulations_main``), from the expense fan-out probe
        (``mcr_probe_expenses_rng``).  Aligned with the input; each value equals, bit for bit,
        ``_success_probability(run_monte_carlo_simulations(working_months, n)[0])`` of a simulator whose config differs
        only in ``monthly_expenses``.  Under a process group the levels go through ``distributed.probe_candidates`` (as
        candidate indices), so every rank returns the same array."""
        return self._level_probabilities(E.probe_expenses, working_months, [float(x) for x in monthly_expenses], num_simulations)

    def find_maximum_monthly_expenses(
        self,
        working_months: int,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
        resolution: float = 1.0,
    ) -> Tuple[float, float, List[Dict[str, float]]]:
        """Largest ``monthly_expenses`` (whole cents) that still reaches ``target_probability`` when retiring after
        ``working_months``: search stream, ``num_simulations_search`` paths, ``MCR_MAX_EXPENSE_FANOUT`` levels per probe
        (`spending.search_maximum_expenses`).  Returns ``(expenses, probability, curve)``; ``expenses == -1.0`` when even
        zero spending misses the target.  Deterministic for a given seed, and the same on every rank."""
        from .spending import EXPENSE_CAP, search_maximum_expenses

        def plan(p, n_sims, target):
            def probe_levels(levels):
                return list(self.success_probability_by_expenses(working_months, levels, n_sims))

            return (f"Searching the maximum monthly expenses at {int(working_months)} working months for '{p.Nickname}' "
                    f"(target {target:.2f}%, {n_sims} sims per level, resolution {resolution}).",
                    lambda: search_maximum_expenses(
                        probe_levels, target, max(float(p.monthly_expenses), 1.0), levels_per_call=N.MCR_MAX_EXPENSE_FANOUT,
                        resolution=resolution, cap=EXPENSE_CAP, on_level=progress_callback),
                    lambda expenses, prob, curve: (expenses >= 0, (
                        f"Target not met even without spending: {prob:.2f}% at {int(working_months)} months." if expenses < 0 else
                        f"  Expense search complete: {expenses:.2f} per month with prob {prob:.2f}% ({len(curve)} levels evaluated).")))

        return self._find_level(verbose, plan)

    def _find_level(self, verbose: bool, plan):
        """The frame of the single-level `find_*` searches.  Switches to the search seeds; ``plan(params_model, paths per level,
        target)`` then gives ``(opening, search, closing)``: the opening log line, the search to run (no arguments; its tuple
        is the result) and ``closing(*result) -> (met, text)``, logged as a line or, when the target was not met, as a warning."""
        self.use_search_seeds()
        p = self.params_model
        opening, search, closing = plan(p, int(p.num_simulations_search), float(p.target_probability))
        if verbose:
            logger.info(opening)
        result = search()
        if verbose:
            met, text = closing(*result)
            (logger.info if met else logger.warning)(text)
        return result

    # ---- spending rules ------------------------------------------------------------------------------
    def _rule_counts(self, working_months: int, rule, params, n: int, multipliers: bool = False) -> np.ndarray:
        """The integers of one launch under `rule` over the active stream's batch of ``n`` paths: the two counters, the
        ``4 ry`` year counts and, with ``multipliers``, the number of paths that were ever cut.  Sharded by PATH RANGE through
        `distributed.probe_candidates` (one all-reduce; every rank returns the same vector)."""
        wm, ry = int(working_months), int(self.params_model.retirement_years)
        rng, dev = self._batch_rng(n), self._local_device()
        width = N.MCR_N_COUNTERS + N.MCR_RULE_N_COUNTS * ry + (1 if multipliers else 0)

        def probe(path_begin, count, _):
            if not multipliers:
                return E.run_rule(params, rng, self._stream_id, path_begin, count, wm, rule, device=dev)["counts"]
            res = E.run_rule_host(params, rng, self._stream_id, path_begin, count, wm, rule, multipliers=True, device=dev)
            with np.errstate(invalid="ignore"):
                ever = int(np.count_nonzero(np.any(res["multipliers"] < 1.0, axis=0)))
            return np.concatenate([res["counters"].astype(np.int64), res["year_counts"].astype(np.int64).reshape(-1), [ever]])

        return D.probe_candidates([0], n, self.shard_min_paths, probe, width=width)[0]

    def success_probability_with_rule(self, working_months: int, rule, monthly_expenses=None,
                                      num_simulations: Optional[int] = None):
        """Success % at ``working_months`` when spending follows `rule` (a `spending_rules.SpendingRule`), over the active
        seed stream's batch of ``num_simulations`` paths (default ``num_simulations_main``).  ``monthly_expenses``: None (the
        config's own level; returns a float), one level (a float) or a sequence of levels (an array aligned with it): the
        spending the path STARTS with.  One level is one launch (``mcr_run_rule_rng``); two or more go through the rule
        probe (``mcr_probe_rules_rng``), up to ``MCR_MAX_EXPENSE_FANOUT`` of them sharing each path's random numbers, and
        count the same integers.  Under the neutral rule each value equals `success_probability_by_expenses` at the same
        level, bit for bit."""
        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        scalar = monthly_expenses is None or np.ndim(monthly_expenses) == 0
        levels = [None] if monthly_expenses is None else [float(x) for x in np.atleast_1d(np.asarray(monthly_expenses, dtype=np.float64))]
        if len(levels) >= 2:
            p = self.params_model
            counts = self._rule_probe_counts(working_months, [(p.initial_balance, p.monthly_contribution, x, rule) for x in levels], n)
            return np.array([self._count_percent(c[N.MCR_CTR_SUCCESS], n) for c in counts], dtype=np.float64)
        out = []
        for level in levels:
            params = params_from_config(self.params_model)     # (a block of this call's own: the level goes into it)
            if level is not None:
                params.monthly_expenses = level
            counts = self._rule_counts(working_months, rule, params, n)
            out.append(self._count_percent(counts[N.MCR_CTR_SUCCESS], n))
        return float(out[0]) if scalar else np.array(out, dtype=np.float64)

    def spending_rule_outcomes(self, working_months: int, rule, num_simulations: Optional[int] = None, multipliers: bool = False):
        """What `rule` does to the plan at ``working_months``: one count-only launch over the active stream's batch returns
        the ``2 + 4 ry`` integers of a `spending_rules.SpendingRuleOutcomes` (success count; per retirement year the paths
        alive, cut, at the floor and raised).  ``multipliers=True`` also downloads the multiplier rows and counts the paths
        that were ever cut (``ever_cut_share``).  Under a process group the integers are summed in one all-reduce and every
        rank returns the same object."""
        from .spending_rules import SpendingRuleOutcomes

        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        ry = int(self.params_model.retirement_years)
        flat = self._rule_counts(working_months, rule, self._current_params(), n, multipliers=bool(multipliers))
        k = N.MCR_N_COUNTERS + N.MCR_RULE_N_COUNTS * ry
        return SpendingRuleOutcomes(int(flat[N.MCR_CTR_SUCCESS]), n, flat[N.MCR_N_COUNTERS:k].reshape(ry, N.MCR_RULE_N_COUNTS),
                                    retirement_age(self.params_model.current_age, int(working_months)),
                                    ever_cut=int(flat[k]) if multipliers else None)

    def spending_rule_fan_chart(self, working_months: int, rule, num_simulations: Optional[int] = None, edges=None, wr_edges=None,
                                m_edges=None) -> Dict[str, object]:
        """The fan charts of a household that follows `rule` at ``working_months``, for any number of paths: one yearly-bins
        launch under the rule over the active stream's batch (``mcr_run_rule_year_bins_rng``; nothing is kept per path, one
        all-reduce under a process group).  Returns the tables of ``distributed.run_sharded_year_bins(rule=...)`` (balance,
        real balance, withdrawal rate, final balance, ``rule_year_counts``, ``multiplier_bins`` and the edges) with
        ``spending`` = the `spending_rules.SpendingBands` of the real monthly spending per retirement year and ``outcomes`` =
        the `spending_rules.SpendingRuleOutcomes` of the year counts."""
        from . import distributed as D
        from .spending_rules import SpendingBands, SpendingRuleOutcomes

        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        if n <= 0:
            raise ValueError("spending_rule_fan_chart needs at least one path")
        params = self._current_params()
        rng = self._batch_rng(n)
        if D.is_active():
            yb = D.run_sharded_year_bins(params, rng, self._stream_id, n, int(working_months), edges, wr_edges, rule=rule, m_edges=m_edges)
        else:
            import torch

            with torch.cuda.device(self._local_device()):
                yb = D.run_sharded_year_bins(params, rng, self._stream_id, n, int(working_months), edges, wr_edges, rule=rule, m_edges=m_edges)
        yb["spending"] = SpendingBands(yb["multiplier_bins"], yb["m_edges"], float(params.monthly_expenses))
        yb["outcomes"] = SpendingRuleOutcomes(int(yb["counters"][0]), n, yb["rule_year_counts"],
                                              retirement_age(self.params_model.current_age, int(working_months)))
        return yb

    def find_maximum_initial_expenses(
        self,
        working_months: int,
        rule,
        resolution: float = 1.0,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
    ) -> Tuple[float, float, List[Dict[str, float]]]:
        """`find_maximum_monthly_expenses` for a household that follows `rule`: the largest ``monthly_expenses`` to START
        retirement with (whole cents) that still reaches ``target_probability``.  The same search
        (`spending.search_maximum_expenses`), stream, path count and return shape, ``-1.0`` when even zero spending misses
        the target; its probe is `success_probability_with_rule`.  With the neutral rule the result is exactly
        `find_maximum_monthly_expenses`'."""
        from .spending import EXPENSE_CAP, search_maximum_expenses

        def plan(p, n_sims, target):
            def probe_levels(levels):
                return list(self.success_probability_with_rule(working_months, rule, list(levels), n_sims))

            return (f"Searching the maximum initial monthly expenses under a spending rule at {int(working_months)} working "
                    f"months for '{p.Nickname}' (target {target:.2f}%, {n_sims} sims per level, resolution {resolution}).",
                    lambda: search_maximum_expenses(
                        probe_levels, target, max(float(p.monthly_expenses), 1.0), levels_per_call=N.MCR_MAX_EXPENSE_FANOUT,
                        resolution=resolution, cap=EXPENSE_CAP, on_level=progress_callback),
                    lambda expenses, prob, curve: (expenses >= 0, (
                        f"Target not met even without spending: {prob:.2f}% at {int(working_months)} months." if expenses < 0 else
                        f"  Rule expense search complete: {expenses:.2f} per month to begin with, prob {prob:.2f}% "
                        f"({len(curve)} levels evaluated).")))

        return self._find_level(verbose, plan)

    # ---- spending rules compared on shared paths ----------------------------------------------------
    def _rule_probe_counts(self, working_months: int, records, n: int) -> np.ndarray:
        """``[len(records), 2 + 4 ry]`` integers of the rule probe (``mcr_probe_rules_rng``) over the active stream's batch
        of ``n`` paths: per record of `spending_rules.rule_options` its two counters and its year counts, row-major.  The
        records go through ``distributed.probe_candidates`` as candidate indices; every rank returns the same array."""
        import torch

        wm, ry = int(working_months), int(self.params_model.retirement_years)
        width = N.MCR_N_COUNTERS + N.MCR_RULE_N_COUNTS * ry
        if not records:
            return np.zeros((0, width), dtype=np.int64)
        params, rng, dev = self._current_params(), self._batch_rng(n), self._local_device()

        def probe(path_begin, count, idx):
            counts, years = E.probe_rules(params, rng, self._stream_id, path_begin, count, wm, [records[i] for i in idx], device=dev)
            return torch.cat([counts, years.reshape(len(idx), -1)], dim=1)

        return D.probe_candidates(list(range(len(records))), n, self.shard_min_paths, probe, width=width)

    def success_probability_by_rules(self, working_months: int, options: Sequence[dict],
                                     num_simulations: Optional[int] = None) -> np.ndarray:
        """Success % of each spending-rule option at ``working_months``, over the active seed stream's batch of
        ``num_simulations`` paths (default ``num_simulations_main``), from the rule probe (``mcr_probe_rules_rng``).  An
        option is a mapping ``{"rule": SpendingRule | six numbers | None, "initial_balance"?, "monthly_contribution"?,
        "monthly_expenses"?}`` (`spending_rules.rule_options`): None is fixed spending, a missing amount takes the config's
        value, an unknown key raises ``ValueError`` (before any device work).  Aligned with the input; each value equals,
        bit for bit, `success_probability_with_rule` of a simulator whose config differs in those amounts only.  Under a
        process group the options go through ``distributed.probe_candidates`` (as candidate indices), so every rank returns
        the same array."""
        from .spending_rules import rule_options

        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        counts = self._rule_probe_counts(working_months, rule_options(self.params_model, options), n)
        return np.array([self._count_percent(c[N.MCR_CTR_SUCCESS], n) for c in counts], dtype=np.float64)

    def joint_outcomes_by_rules(self, working_months: int, options: Sequence[dict], num_simulations: Optional[int] = None):
        """The joint outcomes of the options of `success_probability_by_rules` (same arguments) over their shared paths,
        from the joint rule probe (``mcr_probe_rules_joint_rng``): a `paired.JointOutcomes` whose ``.probabilities`` equal
        that method's array bit for bit.  At most ``MCR_MAX_JOINT_OPTIONS`` options."""
        return self._option_probe("joint", "rules", working_months, options, num_simulations)

    def option_outcomes_by_rules(self, working_months: int, options: Sequence[dict], num_simulations: Optional[int] = None,
                                 quantiles: Sequence[float] = (0.05, 0.25, 0.5, 0.75, 0.95)):
        """The per-option outcomes of the options of `success_probability_by_rules` (same arguments and validation) over
        their shared paths, from the rule outcomes probe (``mcr_probe_rules_outcomes_rng``): an `outcomes.OptionOutcomes`
        whose ``.probabilities`` equal that method's array bit for bit."""
        return self._option_probe("outcomes", "rules", working_months, options, num_simulations, quantiles=quantiles)

    def compare_spending_rules(self, working_months: int, options: Sequence[dict], num_simulations: Optional[int] = None,
                               paired: bool = False, outcomes: bool = False) -> dict:
        """Which guardrail to choose: the options of `success_probability_by_rules` over the same paths as ``{"options":
        [{"initial_balance", "monthly_contribution", "monthly_expenses", "rule": `SpendingRule.as_dict` or None,
        "probability", "years": `SpendingRuleOutcomes.years` of the option}, ...], "best": index}``, ``best`` being the option
        with the highest probability (the first of equals).  ``paired=True`` adds ``"vs_best"`` to every row and
        ``"tied_with_best"``, ``"all_succeed"`` and ``"none_succeed"`` to the document (`joint_outcomes_by_rules`);
        ``outcomes=True`` adds ``"lasts_until_age"``, ``"median_ruin_age"`` and ``"final_balance"`` to every row
        (`option_outcomes_by_rules`) -- both exactly as `compare_claiming_options` adds them, and they compose."""
        from .nestegg import SCENARIO_FIELDS
        from .spending_rules import SpendingRuleOutcomes, rule_options

        records = rule_options(self.params_model, options)
        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        ry = int(self.params_model.retirement_years)
        age = retirement_age(self.params_model.current_age, int(working_months))
        counts = self._rule_probe_counts(working_months, records, n)
        rows = []
        for r, c in zip(records, counts):
            o = SpendingRuleOutcomes(int(c[N.MCR_CTR_SUCCESS]), n, c[N.MCR_N_COUNTERS:].reshape(ry, N.MCR_RULE_N_COUNTS), age)
            rows.append(dict(zip(SCENARIO_FIELDS, r[:3]), rule=None if r[3] is None else r[3].as_dict(),
                             probability=self._count_percent(c[N.MCR_CTR_SUCCESS], n), years=o.years()))
        joint = self.joint_outcomes_by_rules(working_months, options, num_simulations) if paired else None
        per_option = self.option_outcomes_by_rules(working_months, options, num_simulations) if outcomes else None
        return self._best_option_document({}, rows, joint, per_option)

    @staticmethod
    def _best_option_document(head: dict, rows: List[dict], joint, per_option) -> dict:
        """The tail `compare_claiming_options` and `compare_spending_rules` share: ``head`` + ``{"options": rows, "best":
        index of the highest probability (the first of equals)}``; with ``joint`` (a `paired.JointOutcomes`) every row gains
        ``"vs_best"`` and the document ``"tied_with_best"``, ``"all_succeed"`` and ``"none_succeed"``; with ``per_option`` (an
        `outcomes.OptionOutcomes`) every row gains its `OptionOutcomes.row`."""
        best = max(range(len(rows)), key=lambda i: (rows[i]["probability"], -i)) if rows else None
        doc = dict(head, options=rows, best=best)
        if joint is not None:
            for i, row in enumerate(rows):
                row["vs_best"] = joint.difference(best, i)
            doc["tied_with_best"] = joint.indistinguishable_from(best) if rows else []
            doc["all_succeed"], doc["none_succeed"] = joint.all_succeed, joint.none_succeed
        if per_option is not None:
            for i, row in enumerate(rows):
                row.update(per_option.row(i))
        return doc

    # ---- minimum-contribution search ---------------------------------------------------------------
    def success_probability_by_contributions(self, working_months: int, monthly_contributions: Sequence[float],
                                             num_simulations: Optional[int] = None) -> np.ndarray:
        """Success % of each ``monthly_contribution`` level at ``working_months``, over the active seed stream's batch of
        ``num_simulations`` paths (default ``num_simulations_main``), from the contribution fan-out probe
        (``mcr_probe_contributions_rng``).  Aligned with the input; each value equals, bit for bit,
        ``_success_probability(run_monte_carlo_simulations(working_months, n)[0])`` of a simulator whose config differs
        only in ``monthly_contribution``.  Under a process group the levels go through ``distributed.probe_candidates`` (as
        candidate indices), so every rank returns the same array."""
        return self._level_probabilities(E.probe_contributions, working_months, [float(x) for x in monthly_contributions], num_simulations)

    def find_minimum_monthly_contribution(
        self,
        working_months: int,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
        resolution: float = 1.0,
    ) -> Tuple[float, float, List[Dict[str, float]]]:
        """Smallest ``monthly_contribution`` (whole cents) that reaches ``target_probability`` when retiring after
        ``working_months``: search stream, ``num_simulations_search`` paths, ``MCR_MAX_EXPENSE_FANOUT`` levels per probe
        (`saving.search_minimum_contribution`, starting at ``max(monthly_contribution, 1)``).  Returns ``(contribution,
        probability, curve)``; ``contribution == 0.0`` when nothing needs to be saved and ``-1.0`` when even the cap misses
        the target.  At ``working_months == 0`` no contribution is ever made: level 0 is probed once.  Deterministic for a
        given seed, and the same on every rank."""
        from .saving import CONTRIBUTION_CAP, search_minimum_contribution

        def plan(p, n_sims, target):
            wm = int(working_months)

            def probe_levels(levels):
                return list(self.success_probability_by_contributions(wm, levels, n_sims))

            def search():
                if wm != 0:
                    return search_minimum_contribution(
                        probe_levels, target, max(float(p.monthly_contribution), 1.0), levels_per_call=N.MCR_MAX_EXPENSE_FANOUT,
                        resolution=resolution, cap=CONTRIBUTION_CAP, on_level=progress_callback)
                prob = probe_levels([0.0])[0]      # nothing is ever contributed: every level has P(0)
                if progress_callback:
                    progress_callback({"type": "contribution_search_iter", "iteration": 1, "monthly_contribution": 0.0,
                                       "probability": round(prob, 2), "target": target, "lo": None, "hi": None})
                return (0.0 if prob >= target else -1.0), prob, [{"monthly_contribution": 0.0, "probability": prob}]

            return (f"Searching the minimum monthly contribution at {wm} working months for '{p.Nickname}' "
                    f"(target {target:.2f}%, {n_sims} sims per level, resolution {resolution}).", search,
                    lambda contribution, prob, curve: (contribution >= 0, (
                        f"Target not met at any monthly contribution: {prob:.2f}% at {wm} months." if contribution < 0 else
                        f"  Contribution search complete: {contribution:.2f} per month with prob {prob:.2f}% "
                        f"({len(curve)} levels evaluated).")))

        return self._find_level(verbose, plan)

    # ---- what-if scenarios and the required-starting-balance search -----------------------------------
    def success_probability_by_scenarios(self, working_months: int, scenarios: Sequence[dict],
                                         num_simulations: Optional[int] = None) -> np.ndarray:
        """Success % of each what-if scenario at ``working_months``, over the active seed stream's batch of
        ``num_simulations`` paths (default ``num_simulations_main``), from the scenario probe (``mcr_probe_scenarios_rng``).
        A scenario is a mapping with any subset of the keys ``initial_balance``, ``monthly_contribution``,
        ``monthly_expenses``: a missing key takes the config's value, an unknown key raises ``ValueError`` (before any
        device work).  Aligned with the input; each value equals, bit for bit,
        ``_success_probability(run_monte_carlo_simulations(working_months, n)[0])`` of a simulator whose config differs in
        those fields only.  Under a process group the scenarios go through ``distributed.probe_candidates`` (as candidate
        indices), so every rank returns the same array."""
        return self._option_probabilities("scenarios", working_months, scenarios, num_simulations)

    def joint_outcomes_by_scenarios(self, working_months: int, scenarios: Sequence[dict],
                                    num_simulations: Optional[int] = None):
        """The joint outcomes of the scenarios of `success_probability_by_scenarios` (same arguments) over their shared
        paths, from the joint scenario probe (``mcr_probe_scenarios_joint_rng``): a `paired.JointOutcomes` whose
        ``.probabilities`` equal that method's array bit for bit.  At most ``MCR_MAX_JOINT_OPTIONS`` scenarios."""
        return self._option_probe("joint", "scenarios", working_months, scenarios, num_simulations)

    def option_outcomes_by_scenarios(self, working_months: int, scenarios: Sequence[dict], num_simulations: Optional[int] = None,
                                     quantiles: Sequence[float] = (0.05, 0.25, 0.5, 0.75, 0.95)):
        """The per-option outcomes of the scenarios of `success_probability_by_scenarios` (same arguments and validation)
        over their shared paths, from the scenario outcomes probe (``mcr_probe_scenarios_outcomes_rng``): an
        `outcomes.OptionOutcomes` -- ruin-month counts, the `quantiles` of the successful cohort's final balance --
        whose ``.probabilities`` equal that method's array bit for bit."""
        return self._option_probe("outcomes", "scenarios", working_months, scenarios, num_simulations, quantiles=quantiles)

    def find_minimum_initial_balance(
        self,
        working_months: int,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
        resolution: float = 1.0,
    ) -> Tuple[float, float, List[Dict[str, float]]]:
        """Smallest ``initial_balance`` (whole cents) that reaches ``target_probability`` when retiring after
        ``working_months``: search stream, ``num_simulations_search`` paths, ``MCR_MAX_EXPENSE_FANOUT`` levels per probe
        (`nestegg.search_minimum_initial_balance`, starting at ``max(initial_balance, 1)``).  Returns ``(balance,
        probability, curve)``; ``balance == 0.0`` when nothing is needed up front and ``-1.0`` when even the cap misses the
        target.  Valid at ``working_months == 0`` ("retire today"), where the starting balance is the only lever.
        Deterministic for a given seed, and the same on every rank."""
        return self._minimum_initial_balances(working_months, [float(self.params_model.monthly_expenses)], verbose,
                                              progress_callback, resolution, tag_events=False)[0]

    def find_minimum_initial_balance_by_expenses(
        self,
        working_months: int,
        monthly_expenses: Sequence[float],
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
        resolution: float = 1.0,
    ) -> List[Tuple[float, float, List[Dict[str, float]]]]:
        """`find_minimum_initial_balance` at several spending levels at once (the safe-withdrawal-rate curve is ``12 *
        expenses / balance``): one ``(balance, probability, curve)`` per entry of ``monthly_expenses``, each equal to what
        ``find_minimum_initial_balance(working_months)`` returns on a config with that ``monthly_expenses``, for the same
        seed.  The searches run in lockstep (`nestegg.search_minimum_initial_balance_many`): every round is ONE
        `success_probability_by_scenarios` call over the (balance, expenses) points of all unfinished searches, which the
        library takes ``MCR_MAX_EXPENSE_FANOUT`` to a launch.  ``progress_callback`` events also carry
        ``monthly_expenses``."""
        return self._minimum_initial_balances(working_months, monthly_expenses, verbose, progress_callback, resolution,
                                              tag_events=True)

    def _minimum_initial_balances(self, working_months: int, monthly_expenses: Sequence[float], verbose: bool,
                                  progress_callback: Optional[Callable[[dict], None]], resolution: float, tag_events: bool):
        """The body of `find_minimum_initial_balance` (one spending level, the config's, events untagged) and
        `find_minimum_initial_balance_by_expenses`."""
        from .nestegg import INITIAL_BALANCE_CAP, search_minimum_initial_balance_many

        expenses = [float(x) for x in monthly_expenses]
        self.use_search_seeds()
        p = self.params_model
        wm = int(working_months)
        n_sims, target = int(p.num_simulations_search), float(p.target_probability)
        if verbose:
            logger.info(f"Searching the minimum initial balance at {wm} working months for '{p.Nickname}' at "
                        f"{len(expenses)} spending level(s) (target {target:.2f}%, {n_sims} sims per level, resolution {resolution}).")

        def probe_rows(rows, levels_2d):
            points = [{"initial_balance": b, "monthly_expenses": expenses[i]} for i, levels in zip(rows, levels_2d) for b in levels]
            probs = self.success_probability_by_scenarios(wm, points, n_sims).tolist()
            out, at = [], 0
            for levels in levels_2d:
                out.append(probs[at:at + len(levels)])
                at += len(levels)
            return out

        start = max(float(p.initial_balance), 1.0)
        results = search_minimum_initial_balance_many(
            probe_rows, target, [start] * len(expenses), levels_per_call=N.MCR_MAX_EXPENSE_FANOUT, resolution=resolution,
            cap=INITIAL_BALANCE_CAP, on_level=progress_callback, monthly_expenses=expenses if tag_events else None)
        if verbose:
            for e, (balance, prob, curve) in zip(expenses, results):
                if balance < 0:
                    logger.warning(f"Target not met at any initial balance: {prob:.2f}% at {wm} months, {e:.2f} per month.")
                else:
                    logger.info(f"  {e:.2f} per month: initial balance {balance:.2f} with prob {prob:.2f}% "
                                f"({len(curve)} levels evaluated).")
        return results

    # ---- allocation options and the best-split search ---------------------------------------------------
    def success_probability_by_allocations(self, working_months: int, allocations: Sequence,
                                           num_simulations: Optional[int] = None) -> np.ndarray:
        """Success % of each split between the two assets at ``working_months``, over the active seed stream's batch of
        ``num_simulations`` paths (default ``num_simulations_main``), from the allocation probe
        (``mcr_probe_allocations_rng``).  An option is a number (``allocation_inv1_pct``) or a mapping with
        ``allocation_inv1_pct`` and any subset of ``initial_balance``, ``monthly_contribution``, ``monthly_expenses`` (a
        missing amount takes the config's value); a bad option raises ``ValueError`` naming it (before any device work).
        Aligned with the input; each value equals, bit for bit,
        ``_success_probability(run_monte_carlo_simulations(working_months, n)[0])`` of a simulator whose config differs in
        those fields only.  Under a process group the options go through ``distributed.probe_candidates`` (as candidate
        indices), so every rank returns the same array."""
        return self._option_probabilities("allocations", working_months, allocations, num_simulations)

    def joint_outcomes_by_allocations(self, working_months: int, allocations: Sequence, num_simulations: Optional[int] = None):
        """The joint outcomes of the options of `success_probability_by_allocations` (same arguments) over their shared
        paths, from the joint allocation probe (``mcr_probe_allocations_joint_rng``): a `paired.JointOutcomes` whose
        ``.probabilities`` equal that method's array bit for bit.  At most ``MCR_MAX_JOINT_OPTIONS`` options."""
        return self._option_probe("joint", "allocations", working_months, allocations, num_simulations)

    def option_outcomes_by_allocations(self, working_months: int, allocations: Sequence, num_simulations: Optional[int] = None,
                                       quantiles: Sequence[float] = (0.05, 0.25, 0.5, 0.75, 0.95)):
        """The per-option outcomes of the options of `success_probability_by_allocations` (same arguments and validation)
        over their shared paths, from the allocation outcomes probe (``mcr_probe_allocations_outcomes_rng``): an
        `outcomes.OptionOutcomes` whose ``.probabilities`` equal that method's array bit for bit."""
        return self._option_probe("outcomes", "allocations", working_months, allocations, num_simulations, quantiles=quantiles)

    def compare_allocations(self, working_months: int, allocations: Optional[Sequence] = None,
                            num_simulations: Optional[int] = None, paired: bool = False, outcomes: bool = False) -> dict:
        """How to split the money: `success_probability_by_allocations` of ``allocations`` (default: the eleven splits 0, 0.1,
        ..., 1) as ``{"options": [{the three amounts, "allocation_inv1_pct", "probability"}, ...], "best": index}``, ``best``
        being the option with the highest probability (the first of equals).  ``paired=True`` adds ``"vs_best"`` to every row
        and ``"tied_with_best"``, ``"all_succeed"`` and ``"none_succeed"`` to the document (`joint_outcomes_by_allocations`);
        ``outcomes=True`` adds ``"lasts_until_age"``, ``"median_ruin_age"`` and ``"final_balance"`` to every row
        (`option_outcomes_by_allocations`) -- both exactly as `compare_claiming_options` adds them, and they compose."""
        from .allocation import ALLOCATION_OPTION_FIELDS, DEFAULT_ALLOCATIONS, allocation_records

        options = list(DEFAULT_ALLOCATIONS if allocations is None else allocations)
        records = allocation_records(self.params_model, options)
        joint = self.joint_outcomes_by_allocations(working_months, options, num_simulations) if paired else None
        per_option = self.option_outcomes_by_allocations(working_months, options, num_simulations) if outcomes else None
        probs = (joint.probabilities if paired else per_option.probabilities if outcomes else
                 self.success_probability_by_allocations(working_months, options, num_simulations))
        rows = [dict(zip(ALLOCATION_OPTION_FIELDS, r), probability=float(pr)) for r, pr in zip(records, probs)]
        return self._best_option_document({}, rows, joint, per_option)

    def find_best_allocation(
        self,
        working_months: int,
        resolution: float = 0.01,
        num_simulations: Optional[int] = None,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
    ) -> Tuple[float, float, List[Dict[str, float]], List[float]]:
        """The ``allocation_inv1_pct`` (a multiple of ``resolution``) with the highest success probability when retiring after
        ``working_months``: search stream, ``num_simulations`` paths a point (default ``num_simulations_search``),
        ``MCR_MAX_EXPENSE_FANOUT`` splits per probe (`allocation.search_best_allocation`: the grid 0, 0.1, ..., 1, then finer
        grids around the best point; ties go to the split nearest the config's own).  Returns ``(allocation, probability,
        curve, tied)``; ``tied`` are the splits of the first grid (and the answer) that a paired test on the same paths
        cannot tell from the answer.  A refined grid does not promise the global optimum of a noisy curve: read ``tied``.
        Deterministic for a given seed, and the same on every rank."""
        from .allocation import search_best_allocation

        def plan(p, n_search, target):
            wm = int(working_months)
            n_sims = n_search if num_simulations is None else int(num_simulations)

            def search():
                return search_best_allocation(
                    lambda splits: list(self.success_probability_by_allocations(wm, list(splits), n_sims)),
                    float(p.allocation_inv1_pct), resolution=resolution, levels_per_call=N.MCR_MAX_EXPENSE_FANOUT,
                    on_level=progress_callback,
                    probe_joint=lambda splits: self.joint_outcomes_by_allocations(wm, list(splits), n_sims))

            return (f"Searching the best allocation at {wm} working months for '{p.Nickname}' "
                    f"({n_sims} sims per split, resolution {resolution}).", search,
                    lambda allocation, prob, curve, tied: (True, (
                        f"  Allocation search complete: {allocation:.4g} in asset 1 with prob {prob:.2f}% "
                        f"({len(curve)} splits evaluated; {len(tied)} of the first grid indistinguishable from it).")))

        return self._find_level(verbose, plan)

    # ---- glide paths: a split that changes with the calendar ---------------------------------------------
    def success_probability_by_glide_paths(self, working_months: int, glide_paths: Sequence,
                                           num_simulations: Optional[int] = None) -> np.ndarray:
        """Success % of each glide path at ``working_months``, over the active seed stream's batch of ``num_simulations`` paths
        (default ``num_simulations_main``), from the glide probe (``mcr_probe_glide_paths_rng``; include/mcr.h: GLIDE PATH).
        An option is an `allocation.GlidePath`, a sequence of weights by whole years from today, a number (a constant split),
        a string ``start>end@from-to``, or a mapping with ``glide_path`` and any subset of ``initial_balance``,
        ``monthly_contribution``, ``monthly_expenses``; a bad option raises ``ValueError`` naming it (before any device work).
        Aligned with the input; a constant table gives `success_probability_by_allocations`' value for that split bit for bit.
        The NumPy and history streams, stream lists beyond the inline ones and the exact month are not supported under a glide
        path: the library's error is raised unchanged.  Under a process group the options go through
        ``distributed.probe_candidates``, so every rank returns the same array."""
        return self._option_probabilities("glide_paths", working_months, glide_paths, num_simulations)

    def joint_outcomes_by_glide_paths(self, working_months: int, glide_paths: Sequence, num_simulations: Optional[int] = None):
        """The joint outcomes of the options of `success_probability_by_glide_paths` (same arguments) over their shared paths,
        from the joint glide probe (``mcr_probe_glide_paths_joint_rng``): a `paired.JointOutcomes` whose ``.probabilities``
        equal that method's array bit for bit.  At most ``MCR_MAX_JOINT_OPTIONS`` options."""
        return self._option_probe("joint", "glide_paths", working_months, glide_paths, num_simulations)

    def option_outcomes_by_glide_paths(self, working_months: int, glide_paths: Sequence, num_simulations: Optional[int] = None,
                                       quantiles: Sequence[float] = (0.05, 0.25, 0.5, 0.75, 0.95)):
        """The per-option outcomes of the options of `success_probability_by_glide_paths` (same arguments and validation) over
        their shared paths, from the glide outcomes probe (``mcr_probe_glide_paths_outcomes_rng``): an
        `outcomes.OptionOutcomes` whose ``.probabilities`` equal that method's array bit for bit."""
        return self._option_probe("outcomes", "glide_paths", working_months, glide_paths, num_simulations, quantiles=quantiles)

    def compare_glide_paths(self, working_months: int, options: Optional[Sequence] = None, paired: bool = False,
                            outcomes: bool = False, num_simulations: Optional[int] = None) -> dict:
        """How the split should change with age: `success_probability_by_glide_paths` of ``options`` (default:
        `allocation.default_glide_paths` for ``working_months`` -- the config's own constant split, all and none of asset 1, two
        declining target-date shapes and one rising-equity shape) as ``{"options": [{"name", the three amounts, "weights",
        "probability"}, ...], "best": index}``, ``best`` being the option with the highest probability (the first of equals).
        ``paired=True`` and ``outcomes=True`` add what they add to `compare_allocations`, and they compose."""
        from .allocation import SCENARIO_FIELDS, default_glide_paths, glide_paths_of, glide_records

        options = list(default_glide_paths(self.params_model, int(working_months)) if options is None else options)
        records, _ = glide_records(self.params_model, options)
        paths = glide_paths_of(options)
        joint = self.joint_outcomes_by_glide_paths(working_months, options, num_simulations) if paired else None
        per_option = self.option_outcomes_by_glide_paths(working_months, options, num_simulations) if outcomes else None
        probs = (joint.probabilities if paired else per_option.probabilities if outcomes else
                 self.success_probability_by_glide_paths(working_months, options, num_simulations))
        rows = [dict(name=g.describe(), **dict(zip(SCENARIO_FIELDS, r[:3])), weights=list(g.weights), probability=float(pr))
                for g, r, pr in zip(paths, records, probs)]
        return self._best_option_document({}, rows, joint, per_option)

    def _one_glide_path(self, glide_path):
        """The `allocation.GlidePath` of one option as `success_probability_by_glide_paths` takes it (a `GlidePath`, a list, a
        number or a string); ``ValueError`` naming what is wrong with it."""
        from .allocation import glide_paths_of

        if isinstance(glide_path, dict):
            raise ValueError("glide_path: one glide path (a GlidePath, a sequence of weights, a number or a string), not a mapping")
        return glide_paths_of([glide_path])[0]

    def glide_path_fan_chart(self, working_months: int, glide_path, num_simulations: Optional[int] = None, edges=None,
                             wr_edges=None) -> Dict[str, object]:
        """The fan charts of a household that holds `glide_path` at ``working_months``, for any number of paths: one yearly-bins
        launch under the glide path over the active stream's batch (``mcr_run_glide_year_bins_rng``; nothing is kept per path,
        one all-reduce under a process group).  Returns the tables of ``distributed.run_sharded_year_bins(glide_path=...)``
        (balance, real balance, withdrawal rate, final balance and the edges) with ``glide_path`` = ``{"name", "weights"}`` and
        ``allocation_by_sample`` = the weight in force at each yearly sample of `trajectory_time_points`, exact from the table
        (`allocation_by_sample`: the weight of the month each sample closes, ``W[0]`` today)."""
        from . import distributed as D

        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        if n <= 0:
            raise ValueError("glide_path_fan_chart needs at least one path")
        path = self._one_glide_path(glide_path)
        params = self._current_params()
        rng = self._batch_rng(n)
        if D.is_active():
            yb = D.run_sharded_year_bins(params, rng, self._stream_id, n, int(working_months), edges, wr_edges, glide_path=path)
        else:
            import torch

            with torch.cuda.device(self._local_device()):
                yb = D.run_sharded_year_bins(params, rng, self._stream_id, n, int(working_months), edges, wr_edges, glide_path=path)
        yb["glide_path"] = {"name": path.describe(), "weights": list(path.weights)}
        yb["allocation_by_sample"] = allocation_by_sample(path, int(working_months), int(self.params_model.retirement_years))
        return yb

    def glide_path_summary(self, working_months: int, glide_path, num_simulations: Optional[int] = None) -> pd.DataFrame:
        """The reference's per-path summary frame (the columns of `run_monte_carlo_simulations`' ``summary_df``) of the active
        stream's batch of ``num_simulations`` paths under `glide_path`: one summary launch (``mcr_run_glide_rng``) on this
        rank's device.  Its success share equals `success_probability_by_glide_paths`' value for the same option."""
        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        path = self._one_glide_path(glide_path)
        if n <= 0:
            return pd.DataFrame({c: pd.Series(dtype=bool if c == "Success" else np.float64) for c in SUMMARY_COLUMNS})
        res = E.run_glide_host(self._current_params(), self._batch_rng(n), self._stream_id, 0, n, int(working_months), path,
                               want="summary", device=self._local_device())
        cols = {name: res[f] for name, f in _FIELD_OF.items()}
        cols["Success"] = res["success"].astype(np.bool_)
        return pd.DataFrame({c: cols[c] for c in SUMMARY_COLUMNS}, copy=False)

    # ---- income-stream options and the required-income search ------------------------------------------
    def success_probability_by_income_options(self, working_months: int, stream, options: Sequence[dict],
                                              num_simulations: Optional[int] = None) -> np.ndarray:
        """Success % of each option for ONE income stream at ``working_months``, over the active seed stream's batch of
        ``num_simulations`` paths (default ``num_simulations_main``), from the income probe (``mcr_probe_income_rng``).
        ``stream`` is a list index into ``other_income_streams`` or a unique ``name``; an option is a mapping with any subset
        of the keys ``initial_balance``, ``monthly_contribution``, ``monthly_expenses`` and the stream's
        ``monthly_amount_today``, ``start_at_age``, ``duration_years``: a missing key takes the config's value, an unknown
        key or stream raises ``ValueError`` (before any device work).  Aligned with the input; each value equals, bit for
        bit, ``_success_probability(run_monte_carlo_simulations(working_months, n)[0])`` of a simulator whose config differs
        in those fields only.  Under a process group the options go through ``distributed.probe_candidates`` (as candidate
        indices), so every rank returns the same array."""
        return self._option_probabilities("income", working_months, options, num_simulations, stream)

    def joint_outcomes_by_income_options(self, working_months: int, stream, options: Sequence[dict],
                                         num_simulations: Optional[int] = None):
        """The joint outcomes of the options of `success_probability_by_income_options` (same arguments) over their shared
        paths, from the joint income probe (``mcr_probe_income_joint_rng``): a `paired.JointOutcomes` whose
        ``.probabilities`` equal that method's array bit for bit.  At most ``MCR_MAX_JOINT_OPTIONS`` options."""
        return self._option_probe("joint", "income", working_months, options, num_simulations, stream)

    def option_outcomes_by_income_options(self, working_months: int, stream, options: Sequence[dict],
                                          num_simulations: Optional[int] = None,
                                          quantiles: Sequence[float] = (0.05, 0.25, 0.5, 0.75, 0.95)):
        """The per-option outcomes of the options of `success_probability_by_income_options` (same arguments and
        validation) over their shared paths, from the income outcomes probe (``mcr_probe_income_outcomes_rng``): an
        `outcomes.OptionOutcomes` whose ``.probabilities`` equal that method's array bit for bit."""
        return self._option_probe("outcomes", "income", working_months, options, num_simulations, stream, quantiles)

    def compare_claiming_options(self, working_months: int, stream, options: Sequence[dict],
                                 num_simulations: Optional[int] = None, paired: bool = False, outcomes: bool = False) -> dict:
        """The claim-age table and the annuity comparison: `success_probability_by_income_options` of ``options`` as
        ``{"stream": list index, "options": [{the six fields, "probability"}, ...], "best": index}``, ``best`` being the
        option with the highest probability (the first of equals).

        ``paired=True`` says whether the gaps are real: the table comes from `joint_outcomes_by_income_options` (the same
        probabilities), every row gains ``"vs_best"`` = `JointOutcomes.difference` of the best option against the row
        (``delta``, paired ``se``, ``se_unpaired``, McNemar ``p_value``, ``rescued``), and the document gains
        ``"tied_with_best"`` (the rows the paired test cannot tell from the best at 5 %) and ``"all_succeed"`` /
        ``"none_succeed"``, the paths on which every option works and on which none does.

        ``outcomes=True`` says when it goes wrong and what is left: `option_outcomes_by_income_options` over the same paths
        (the same probabilities) adds to every row ``"lasts_until_age"`` = ``{"90", "95", "99"}`` (the age the money lasts
        to with that confidence; None = the whole horizon), ``"median_ruin_age"`` (among the failing paths; None without
        any) and ``"final_balance"`` = ``{"p5", "p25", "p50", "p75", "p95"}`` of the successful paths' nominal final
        balance (None values for an empty cohort).  Composes with ``paired``."""
        from .income import INCOME_OPTION_FIELDS, income_options, stream_index

        index = stream_index(self.params_model, stream)
        records = income_options(self.params_model, index, options)
        joint = self.joint_outcomes_by_income_options(working_months, index, options, num_simulations) if paired else None
        per_option = self.option_outcomes_by_income_options(working_months, index, options, num_simulations) if outcomes else None
        probs = (joint.probabilities if paired else per_option.probabilities if outcomes else
                 self.success_probability_by_income_options(working_months, index, options, num_simulations))
        rows = [dict(zip(INCOME_OPTION_FIELDS, r), probability=float(pr)) for r, pr in zip(records, probs)]
        return self._best_option_document({"stream": index}, rows, joint, per_option)

    _UNCHANGED = object()   # (find_minimum_income_amount: "the stream's own duration_years", which may itself be None)

    def find_minimum_income_amount(
        self,
        working_months: int,
        stream,
        start_at_age: Optional[float] = None,
        duration_years=_UNCHANGED,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
        resolution: float = 1.0,
    ) -> Tuple[float, float, List[Dict[str, float]]]:
        """Smallest ``monthly_amount_today`` (whole cents) of income stream ``stream`` that reaches ``target_probability``
        when retiring after ``working_months``: search stream, ``num_simulations_search`` paths, ``MCR_MAX_EXPENSE_FANOUT``
        levels per probe (`income.search_minimum_income_amount`, starting at ``max(the stream's amount, 1)``).
        ``start_at_age`` / ``duration_years`` replace the stream's own for every level (default: unchanged; ``None`` as
        ``duration_years`` = for life).  Returns ``(amount, probability, curve)``; ``amount == 0.0`` when the plan needs no
        such income and ``-1.0`` when even the cap misses the target.  Deterministic for a given seed, and the same on every
        rank."""
        from .income import INCOME_AMOUNT_CAP, search_minimum_income_amount, stream_index

        def plan(p, n_sims, target):
            wm = int(working_months)
            index = stream_index(p, stream)
            fixed = {}
            if start_at_age is not None:
                fixed["start_at_age"] = float(start_at_age)
            if duration_years is not self._UNCHANGED:
                fixed["duration_years"] = duration_years

            def probe_levels(levels):
                return list(self.success_probability_by_income_options(
                    wm, index, [dict(fixed, monthly_amount_today=x) for x in levels], n_sims))

            return (f"Searching the minimum monthly amount of income stream {index} at {wm} working months for "
                    f"'{p.Nickname}' (target {target:.2f}%, {n_sims} sims per level, resolution {resolution}).",
                    lambda: search_minimum_income_amount(
                        probe_levels, target, max(float(p.other_income_streams[index].monthly_amount_today), 1.0),
                        levels_per_call=N.MCR_MAX_EXPENSE_FANOUT, resolution=resolution, cap=INCOME_AMOUNT_CAP, on_level=progress_callback),
                    lambda amount, prob, curve: (amount >= 0, (
                        f"Target not met at any amount of income stream {index}: {prob:.2f}% at {wm} months." if amount < 0 else
                        f"  Income search complete: {amount:.2f} per month with prob {prob:.2f}% ({len(curve)} levels evaluated).")))

        return self._find_level(verbose, plan)

    # ---- market-assumption stress and the break-even assumption search ---------------------------------
    def success_probability_by_assumptions(self, working_months: int, scenarios: Sequence[dict],
                                           num_simulations: Optional[int] = None) -> np.ndarray:
        """Success % of each record of market assumptions at ``working_months``, over the active seed stream's batch of
        ``num_simulations`` paths (default ``num_simulations_main``), from the assumption probe
        (``mcr_probe_assumptions_rng``).  A record is a mapping with any subset of `stress.ASSUMPTION_FIELDS` (the seven
        market names of `Config` and the three scenario levers): a missing key takes the config's value; an unknown key or
        a value outside `Config`'s bounds raises ``ValueError`` naming ``scenarios[k]`` (before any device work).  Aligned
        with the input; each value equals, bit for bit, ``_success_probability(run_monte_carlo_simulations(working_months,
        n)[0])`` of a simulator whose config differs in those fields only.  Under a process group the records go through
        ``distributed.probe_candidates`` (as candidate indices), so every rank returns the same array."""
        return self._option_probabilities("assumptions", working_months, scenarios, num_simulations)

    def joint_outcomes_by_assumptions(self, working_months: int, scenarios: Sequence[dict],
                                      num_simulations: Optional[int] = None):
        """The joint outcomes of the records of `success_probability_by_assumptions` (same arguments) over their shared
        paths, from the joint assumption probe (``mcr_probe_assumptions_joint_rng``): a `paired.JointOutcomes` whose
        ``.probabilities`` equal that method's array bit for bit.  At most ``MCR_MAX_JOINT_OPTIONS`` records."""
        return self._option_probe("joint", "assumptions", working_months, scenarios, num_simulations)

    def option_outcomes_by_assumptions(self, working_months: int, scenarios: Sequence[dict], num_simulations: Optional[int] = None,
                                       quantiles: Sequence[float] = (0.05, 0.25, 0.5, 0.75, 0.95)):
        """The per-option outcomes of the records of `success_probability_by_assumptions` (same arguments and validation)
        over their shared paths, from the assumption outcomes probe (``mcr_probe_assumptions_outcomes_rng``): an
        `outcomes.OptionOutcomes` whose ``.probabilities`` equal that method's array bit for bit."""
        return self._option_probe("outcomes", "assumptions", working_months, scenarios, num_simulations, quantiles=quantiles)

    def stress_test(self, working_months: int, shifts: Optional[Sequence[Tuple[str, dict]]] = None,
                    num_simulations: Optional[int] = None, paired: bool = False, outcomes: bool = False) -> List[Dict[str, object]]:
        """The stress table at ``working_months``: ONE `success_probability_by_assumptions` call over the base case and one
        row per shift (default `stress.DEFAULT_SHIFTS`: 14 one-at-a-time additive shifts of the market's means,
        volatilities and correlation, i.e. 15 records, one launch).  ``shifts`` replaces the table with ``[(label, {field:
        delta, ...}), ...]``; several fields in one entry make a combined scenario.  Each shifted value is clipped to
        `Config`'s bounds.  Returns ``{"label", "overrides", "probability", "delta"}`` per row, base first: ``overrides``
        holds the applied values, ``delta`` the row's probability minus the base row's, in points.

        ``paired=True``: the table comes from `joint_outcomes_by_assumptions` (the same probabilities) and every row gains
        ``"vs_base"`` = `JointOutcomes.difference` of the base row against it plus ``hurt`` (paths that succeed under the
        base and fail under the shift) and ``helped`` (the reverse).

        ``outcomes=True``: `option_outcomes_by_assumptions` over the same paths (the same probabilities) adds
        ``"lasts_until_age"``, ``"median_ruin_age"`` and ``"final_balance"`` to every row, as in
        `compare_claiming_options`.  Composes with ``paired``."""
        from .stress import stress_scenarios

        rows = stress_scenarios(self.params_model, shifts)
        records = [o for _, o in rows]
        joint = self.joint_outcomes_by_assumptions(working_months, records, num_simulations) if paired else None
        per_option = self.option_outcomes_by_assumptions(working_months, records, num_simulations) if outcomes else None
        probs = (joint.probabilities if paired else per_option.probabilities if outcomes else
                 self.success_probability_by_assumptions(working_months, records, num_simulations))
        base = float(probs[0])
        table = [{"label": label, "overrides": dict(o), "probability": float(pr), "delta": float(pr) - base}
                 for (label, o), pr in zip(rows, probs)]
        if paired:
            for i, row in enumerate(table):
                t = joint.pair(0, i)
                row["vs_base"] = dict(joint.difference(0, i), hurt=t["only_a"], helped=t["only_b"])
        if outcomes:
            for i, row in enumerate(table):
                row.update(per_option.row(i))
        return table

    def find_breakeven_assumption(
        self,
        working_months: int,
        field: str,
        window: float = 0.25,
        resolution: float = 1e-4,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
    ) -> Tuple[Optional[float], float, List[Dict[str, float]], str]:
        """The most adverse value of one mean or volatility of the market (`stress.ADVERSE_DIRECTION`: lower for the two
        return means, higher for the inflation mean and every volatility) at which ``target_probability`` is still met when
        retiring after ``working_months``: search stream, ``num_simulations_search`` paths, ``MCR_MAX_EXPENSE_FANOUT``
        levels per probe (`stress.search_breakeven`).  Levels are multiples of ``resolution`` inside ``[config value -
        window, config value + window]`` clipped to `Config`'s bounds.  Returns ``(value, probability, curve, status)``
        with ``status`` ``"found"``, ``"holds_at_window_end"`` (the value is the window's adverse end) or ``"not_reached"``
        (``None``).  Deterministic for a given seed, and the same on every rank."""
        from .stress import search_breakeven

        def plan(p, n_sims, target):
            wm = int(working_months)

            def probe_levels(values):
                return list(self.success_probability_by_assumptions(wm, [{field: v} for v in values], n_sims))

            return (f"Searching the break-even {field} at {wm} working months for '{p.Nickname}' "
                    f"(target {target:.2f}%, {n_sims} sims per level, window {window}, resolution {resolution}).",
                    lambda: search_breakeven(probe_levels, target, field, float(getattr(p, field)), window=window, resolution=resolution,
                                             levels_per_call=N.MCR_MAX_EXPENSE_FANOUT, on_level=progress_callback),
                    lambda value, prob, curve, status: (status != "not_reached", (
                        f"Target not met at any {field} of the window: {prob:.2f}% at its favourable end." if status == "not_reached" else
                        f"  Break-even search complete ({status}): {field} = {value:.4f} with prob {prob:.2f}% "
                        f"({len(curve)} levels evaluated).")))

        return self._find_level(verbose, plan)

    def _grid_probabilities(self, working_months: Sequence[int], levels_2d: Sequence[Sequence[float]],
                            num_simulations: int, rule=None) -> np.ndarray:
        """Success % ``[len(working_months), n_levels]`` of month ``c`` at the levels of row ``c`` (rectangular), over the
        active stream's batch, from the grid probe (``mcr_probe_grid_rng``) or, with `rule`, from the rule-grid probe
        (``mcr_probe_rule_grid_rng``, its counters alone).  Under a process group the rows go through
        ``distributed.probe_candidates`` (candidate = row, ``2 n_levels`` counters each): one all-reduce, the same matrix
        on every rank."""
        months = [int(m) for m in working_months]
        rows = [[float(x) for x in r] for r in levels_2d]
        n_levels = len(rows[0]) if rows else 0
        if not months or n_levels == 0:
            return np.zeros((len(months), n_levels), dtype=np.float64)
        n = int(num_simulations)
        params, rng, dev = self._current_params(), self._batch_rng(n), self._local_device()

        def probe(path_begin, count, idx):
            if rule is not None:
                return E.probe_rule_grid(params, rng, self._stream_id, path_begin, count, [months[i] for i in idx],
                                         [rows[i] for i in idx], rule, device=dev, year_counts=False)[0]
            return E.probe_grid(params, rng, self._stream_id, path_begin, count, [months[i] for i in idx],
                                [rows[i] for i in idx], device=dev)

        counts = D.probe_candidates(list(range(len(months))), n, self.shard_min_paths, probe,
                                    width=n_levels * N.MCR_N_COUNTERS).reshape(len(months), n_levels, N.MCR_N_COUNTERS)
        return np.array([[self._count_percent(counts[c, k, N.MCR_CTR_SUCCESS], n)
                          for k in range(n_levels)] for c in range(len(months))], dtype=np.float64).reshape(len(months), n_levels)

    def success_probability_grid(self, working_months: Sequence[int], monthly_expenses: Sequence[float],
                                 num_simulations: Optional[int] = None) -> np.ndarray:
        """Success % of every (working month, ``monthly_expenses`` level) pair over the active seed stream's batch of
        ``num_simulations`` paths (default ``num_simulations_main``): ``[len(working_months), len(monthly_expenses)]``.  Row
        ``c`` equals, bit for bit, ``success_probability_by_expenses(working_months[c], monthly_expenses)``; the
        accumulation runs once for all months (``mcr_probe_grid_rng``).  The same matrix on every rank."""
        months = [int(m) for m in working_months]
        levels = [float(x) for x in monthly_expenses]
        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        return self._grid_probabilities(months, [levels] * len(months), n)

    def _rule_grid_probabilities(self, working_months: Sequence[int], levels_2d: Sequence[Sequence[float]], rule,
                                 num_simulations: int) -> np.ndarray:
        """`_grid_probabilities` under `rule` (a `spending_rules.SpendingRule`)."""
        if rule is None:
            raise ValueError("a spending rule is required (SpendingRule.neutral() is fixed spending)")
        return self._grid_probabilities(working_months, levels_2d, num_simulations, rule=rule)

    def success_probability_grid_with_rule(self, working_months: Sequence[int], rule, monthly_expenses=None,
                                           num_simulations: Optional[int] = None) -> np.ndarray:
        """`success_probability_grid` for a household that follows `rule`: ``[len(working_months), n_levels]`` success %,
        ``monthly_expenses`` the levels the paths START retirement with (None: one column at the config's own level).  Row
        ``c`` equals, bit for bit, ``success_probability_with_rule(working_months[c], rule, monthly_expenses)``; a rule
        acts only after retirement, so the accumulation runs once for all months (``mcr_probe_rule_grid_rng``).  The same
        matrix on every rank."""
        months = [int(m) for m in working_months]
        levels = ([float(self.params_model.monthly_expenses)] if monthly_expenses is None
                  else [float(x) for x in np.atleast_1d(np.asarray(monthly_expenses, dtype=np.float64))])
        n = int(self.params_model.num_simulations_main if num_simulations is None else num_simulations)
        return self._rule_grid_probabilities(months, [levels] * len(months), rule, n)

    def find_maximum_initial_expenses_by_months(
        self,
        working_months: Sequence[int],
        rule,
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
        resolution: float = 1.0,
    ) -> List[Tuple[float, float, List[Dict[str, float]]]]:
        """`find_maximum_monthly_expenses_by_months` for a household that follows `rule`: the frontier of the spending to
        START retirement with.  Entry ``i`` equals ``find_maximum_initial_expenses(working_months[i], rule)`` for the same
        seed; every round of the lockstep searches is ONE rule-grid probe over the unfinished months' levels."""
        return self._maximum_expenses_by_months(
            working_months, verbose, progress_callback, resolution, "initial monthly expenses under a spending rule",
            lambda months, levels_2d, n_sims: self._rule_grid_probabilities(months, levels_2d, rule, n_sims))

    def find_maximum_monthly_expenses_by_months(
        self,
        working_months: Sequence[int],
        verbose: bool = True,
        progress_callback: Optional[Callable[[dict], None]] = None,
        resolution: float = 1.0,
    ) -> List[Tuple[float, float, List[Dict[str, float]]]]:
        """`find_maximum_monthly_expenses` for several retirement months at once (the max-spending frontier): one
        ``(expenses, probability, curve)`` per entry of ``working_months``, each equal to what
        ``find_maximum_monthly_expenses(working_months[i])`` returns for the same seed.  The searches run in lockstep
        (`spending.search_maximum_expenses_many`): every round is ONE grid probe over the unfinished months' levels.
        ``progress_callback`` events also carry ``working_months``."""
        return self._maximum_expenses_by_months(working_months, verbose, progress_callback, resolution, "monthly expenses",
                                                self._grid_probabilities)

    def _maximum_expenses_by_months(self, working_months: Sequence[int], verbose: bool, progress_callback, resolution: float,
                                    what: str, grid_probabilities):
        """The frame of the frontier searches: ``grid_probabilities(months, levels_2d, n) -> [rows, levels]`` success %."""
        from .spending import EXPENSE_CAP, search_maximum_expenses_many

        months = [int(m) for m in working_months]
        self.use_search_seeds()
        p = self.params_model
        n_sims, target = int(p.num_simulations_search), float(p.target_probability)
        if verbose:
            logger.info(f"Searching the maximum {what} at {len(months)} retirement months for '{p.Nickname}' "
                        f"(target {target:.2f}%, {n_sims} sims per level, resolution {resolution}).")

        def probe_rows(rows, levels_2d):
            return np.asarray(grid_probabilities([months[i] for i in rows], levels_2d, n_sims)).tolist()

        start = max(float(p.monthly_expenses), 1.0)
        results = search_maximum_expenses_many(
            probe_rows, target, [start] * len(months), levels_per_call=N.MCR_MAX_EXPENSE_FANOUT, resolution=resolution,
            cap=EXPENSE_CAP, on_level=progress_callback, working_months=months)
        if verbose:
            for m, (expenses, prob, curve) in zip(months, results):
                if expenses < 0:
                    logger.warning(f"Target not met even without spending: {prob:.2f}% at {m} months.")
                else:
                    logger.info(f"  {m} months: {expenses:.2f} per month with prob {prob:.2f}% ({len(curve)} levels evaluated).")
        return results


#: the engine's own batch driver: the search takes the count-only fast path only while this is what a call reaches
_ENGINE_RUN = RetirementMonteCarloSimulator.run_monte_carlo_simulations


def _seed_from_timestamp() -> int:
    """Seed when none is configured: hash of the UTC timestamp (backend/utils.py:16-18)."""
    import datetime as _dt
    import hashlib

    ts = _dt.datetime.now(_dt.timezone.utc).isoformat()
    return int.from_bytes(hashlib.sha256(ts.encode()).digest()[:8], "big") % (2**32 - 1)
