"""ctypes binding of the C ABI declared in include/mcr.h (``csrc/libmcr_hip.so``).

This is the only door into the HIP kernels.  There is no CPU fallback: if the shared
library is missing, or no HIP device is usable, the compute entry points raise
``RuntimeError`` — loudly, by design.
"""

from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

MCR_ABI_VERSION = 8
MCR_INLINE_STREAMS = 16  # other_income_streams records inside mcr_params; the rest follow through extra_streams
MCR_N_COUNTERS = 2
MCR_N_STAT_ROWS = 4
MCR_CTR_SUCCESS = 0
MCR_CTR_PATHS = 1
MCR_STREAM_SEARCH = 0
MCR_STREAM_FINAL = 1
MCR_RNG_PHILOX = 0
MCR_RNG_NUMPY = 1
MCR_RNG_HISTORY = 2
MCR_MAX_ENTROPY_WORDS = 8
MCR_MAX_HISTORY_MONTHS = 2048
MCR_HISTORY_BLOCK = 0
MCR_HISTORY_STATIONARY = 1
MCR_HISTORY_COHORTS = 2
MCR_DEVICE_ALL = -2
MCR_MAX_HIST_BINS = 4096
MCR_MAX_YEAR_BINS = 512  # bins per row of the yearly-bins tables (mcr_year_bins)
MCR_ERR_INVALID_ARG = -1
MCR_ERR_NO_DEVICE = -2
MCR_ERR_UNSUPPORTED = -4
MCR_RULE_ALIVE, MCR_RULE_CUT, MCR_RULE_FLOOR, MCR_RULE_RAISED = 0, 1, 2, 3   # columns of mcr_rule_outputs.year_counts
MCR_RULE_N_COUNTS = 4
MCR_MAX_JOINT_OPTIONS = 32  # options of one joint probe / mcr_joint_counts call
MCR_MAX_EXPENSE_FANOUT = 15  # spending levels one expense fan-out workgroup evaluates (mcr_probe_expenses_rng)

MCR_HELPER_WITHDRAW = 0
MCR_HELPER_NLV = 1
MCR_HELPER_REBALANCE = 2
MCR_HELPER_ANNUAL_TAX = 3
MCR_HELPER_MONTHLY_GROSS = 4
MCR_HELPER_MATH_EXP = 5
MCR_HELPER_MATH_DIV = 6
MCR_HELPER_MATH_SQRT = 7
MCR_HELPER_MATH_NEG2LOG = 8
MCR_HELPER_MATH_SINCOS = 9
MCR_HELPER_MATH_DIV_PATH = 10
MCR_HELPER_WITHDRAW2_PATH = 11
MCR_HELPER_NLV2_PATH = 12
MCR_HELPER_REBALANCE_PATH = 13
MCR_HELPER_ANNUAL_TAX_PATH = 14
MCR_HELPER_MATH_EXP_PATH = 15
MCR_HELPER_MATH_NEG2LOG_PATH = 16
MCR_HELPER_MATH_SINCOS_PATH = 17
MCR_HELPER_WITHDRAW_MONTH = 18
MCR_HELPER_REBALANCE_MONTH = 19
MCR_HELPER_MATH_EXP_FORMS = 20
_HELPER_ARITY = {  # which -> (n_in, n_out)
    MCR_HELPER_WITHDRAW: (5, 4),
    MCR_HELPER_NLV: (4, 1),
    MCR_HELPER_REBALANCE: (4, 4),
    MCR_HELPER_ANNUAL_TAX: (6, 5),
    MCR_HELPER_MONTHLY_GROSS: (3, 1),
    MCR_HELPER_MATH_EXP: (1, 1),
    MCR_HELPER_MATH_DIV: (2, 1),
    MCR_HELPER_MATH_SQRT: (1, 1),
    MCR_HELPER_MATH_NEG2LOG: (1, 1),
    MCR_HELPER_MATH_SINCOS: (1, 2),
    MCR_HELPER_MATH_DIV_PATH: (2, 1),
    MCR_HELPER_WITHDRAW2_PATH: (6, 8),
    MCR_HELPER_NLV2_PATH: (4, 2),
    MCR_HELPER_REBALANCE_PATH: (4, 4),
    MCR_HELPER_ANNUAL_TAX_PATH: (6, 5),
    MCR_HELPER_MATH_EXP_PATH: (1, 1),
    MCR_HELPER_MATH_NEG2LOG_PATH: (1, 1),
    MCR_HELPER_MATH_SINCOS_PATH: (1, 2),
    MCR_HELPER_WITHDRAW_MONTH: (5, 6),
    MCR_HELPER_REBALANCE_MONTH: (4, 4),
    MCR_HELPER_MATH_EXP_FORMS: (1, 2),
}


#: include/mcr.h: mcr_reduce_fn — int (*)(void* ctx, void* device_buf, int64_t count, int32_t dtype)
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)
MCR_DT_I32, MCR_DT_I64 = 0, 1


class McrStream(C.Structure):
    _fields_ = [
        ("monthly_amount_today", C.c_double),
        ("start_at_age", C.c_double),
        ("tax_rate", C.c_double),
        ("duration_years", C.c_int32),
        ("inflation_indexed", C.c_int32),
    ]


class McrParams(C.Structure):
    _fields_ = [
        ("initial_balance", C.c_double),
        ("monthly_contribution", C.c_double),
        ("contribution_growth_rate_annual", C.c_double),
        ("monthly_expenses", C.c_double),
        ("current_age", C.c_double),
        ("allocation_inv1_pct", C.c_double),
        ("inv1_annual_tax_on_gains_rate", C.c_double),
        ("inv1_realized_gains_tax_rate", C.c_double),
        ("inv2_annual_tax_on_gains_rate", C.c_double),
        ("inv2_realized_gains_tax_rate", C.c_double),
        ("inv1_mu_log", C.c_double),
        ("inv1_sigma_log", C.c_double),
        ("inf_mu_log", C.c_double),
        ("inf_sigma_log", C.c_double),
        ("prem_mu_log", C.c_double),
        ("prem_sigma_log", C.c_double),
        ("equity_inflation_rho", C.c_double),
        ("retirement_years", C.c_int32),
        ("inv1_use_realized_gains_tax_system", C.c_int32),
        ("inv2_use_realized_gains_tax_system", C.c_int32),
        ("n_streams", C.c_int32),
        ("streams", McrStream * MCR_INLINE_STREAMS),
        ("extra_streams", C.POINTER(McrStream)),
    ]

    #: the ctypes array `extra_streams` points into (a Structure keeps no reference to what its pointer fields point at)
    _extra_keepalive = None

    def set_streams(self, records) -> None:
        """Fill the stream list from `(monthly_amount_today, start_at_age, tax_rate, duration_years, inflation_indexed)`
        tuples — ANY number of them (backend/config.py:99 has no limit): the first MCR_INLINE_STREAMS go into the block, the
        rest into an array this object keeps alive and `extra_streams` points at."""
        records = list(records)
        self.n_streams = len(records)
        extra = (McrStream * max(0, len(records) - MCR_INLINE_STREAMS))()
        for i, (amount, start_age, tax_rate, duration_years, indexed) in enumerate(records):
            s = self.streams[i] if i < MCR_INLINE_STREAMS else extra[i - MCR_INLINE_STREAMS]
            s.monthly_amount_today = amount
            s.start_at_age = start_age
            s.tax_rate = tax_rate
            s.duration_years = -1 if duration_years is None else int(duration_years)
            s.inflation_indexed = int(bool(indexed))
        self._extra_keepalive = extra if len(extra) else None
        self.extra_streams = C.cast(extra, C.POINTER(McrStream)) if len(extra) else C.POINTER(McrStream)()

    def stream(self, i: int) -> McrStream:
        """Entry i of the list, wherever it lives."""
        return self.streams[i] if i < MCR_INLINE_STREAMS else self.extra_streams[i - MCR_INLINE_STREAMS]


class McrRng(C.Structure):
    """Random-stream descriptor (include/mcr.h: mcr_rng)."""

    _fields_ = [
        ("kind", C.c_uint32),
        ("n_entropy_words", C.c_uint32),
        ("entropy", C.c_uint32 * MCR_MAX_ENTROPY_WORDS),
        ("philox_seed", C.c_uint64),
        ("child_offset", C.c_uint64),
        ("path_seeds", C.c_void_p),
        ("history", C.c_void_p),
        ("history_months", C.c_uint32),
        ("history_block", C.c_uint32),
        ("history_scheme", C.c_uint32),
        ("history_reserved", C.c_uint32),
    ]


def philox_rng(seed: int) -> McrRng:
    r = McrRng()
    r.kind = MCR_RNG_PHILOX
    r.philox_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return r


def numpy_rng(main_seed: int, child_offset: int = 0, path_seeds_ptr: int = 0) -> McrRng:
    """The reference's NumPy stream for `main_seed` (SeedSequence entropy words, least significant first)."""
    words, s = [], int(main_seed)
    if s < 0:
        raise ValueError("seed must be nonnegative")
    while True:
        words.append(s & 0xFFFFFFFF)
        s >>= 32
        if s == 0:
            break
    if len(words) > MCR_MAX_ENTROPY_WORDS:
        raise ValueError(f"numpy rng: seeds above {32 * MCR_MAX_ENTROPY_WORDS} bits are not supported")
    r = McrRng()
    r.kind = MCR_RNG_NUMPY
    r.n_entropy_words = len(words)
    for i, w in enumerate(words):
        r.entropy[i] = w
    r.child_offset = int(child_offset)
    r.path_seeds = path_seeds_ptr or None
    return r


def history_rng(seed: int, table, block: int, scheme: int = 0) -> McrRng:
    """The block bootstrap of a recorded market (include/mcr.h: MCR_RNG_HISTORY): ``table`` = Z[months][3] standard shocks
    (equity, inflation, premium), ``block`` = months per block, ``seed`` = the Philox key of the block starts, ``scheme`` =
    MCR_HISTORY_BLOCK (fixed blocks), MCR_HISTORY_STATIONARY (geometric block lengths of mean ``block``) or
    MCR_HISTORY_COHORTS (path i starts at month i mod months; neither ``seed`` nor ``block`` is read).  The
    descriptor points at HOST memory — what the ``*_host_rng`` entry points take — and keeps the array alive as
    ``_history_table``; ``engine`` swaps in a device copy for the entry points that want one."""
    import numpy as np

    z = np.ascontiguousarray(table, dtype=np.float64)
    if z.ndim != 2 or z.shape[1] != 3:
        raise ValueError(f"history table: shape {z.shape} is not (months, 3)")
    if not 1 <= z.shape[0] <= MCR_MAX_HISTORY_MONTHS:
        raise ValueError(f"history table: {z.shape[0]} months (1..{MCR_MAX_HISTORY_MONTHS})")
    if not 1 <= int(block) <= 2**31 - 1:
        raise ValueError(f"history block: {block} months (1..2^31 - 1)")
    if not np.all(np.isfinite(z)):
        raise ValueError("history table: every entry must be finite")
    if isinstance(scheme, bool) or scheme not in (MCR_HISTORY_BLOCK, MCR_HISTORY_STATIONARY, MCR_HISTORY_COHORTS):
        raise ValueError(f"history scheme: {scheme!r} (0 block, 1 stationary, 2 cohorts)")
    r = McrRng()
    r.kind = MCR_RNG_HISTORY
    r.philox_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r.history = z.ctypes.data
    r.history_months = z.shape[0]
    r.history_block = int(block)
    r.history_scheme = int(scheme)
    r._history_table = z
    return r


class McrScenario(C.Structure):
    """One record of a scenario probe (include/mcr.h: mcr_scenario): the three levers success is monotone in."""

    _fields_ = [
        ("initial_balance", C.c_double),
        ("monthly_contribution", C.c_double),
        ("monthly_expenses", C.c_double),
    ]


class McrAssumptions(C.Structure):
    """One record of an assumption probe (include/mcr.h: mcr_assumptions): the three scenario levers and the market's seven
    lognormal parameters, i.e. the ten fields of mcr_params the record replaces."""

    _fields_ = [
        ("initial_balance", C.c_double),
        ("monthly_contribution", C.c_double),
        ("monthly_expenses", C.c_double),
        ("inv1_mu_log", C.c_double),
        ("inv1_sigma_log", C.c_double),
        ("inf_mu_log", C.c_double),
        ("inf_sigma_log", C.c_double),
        ("prem_mu_log", C.c_double),
        ("prem_sigma_log", C.c_double),
        ("equity_inflation_rho", C.c_double),
    ]


class McrIncomeOption(C.Structure):
    """One record of an income probe (include/mcr.h: mcr_income_option): the three scenario levers and the amount, start age
    and duration (-1 = None) of the one income stream the probe varies."""

    _fields_ = [
        ("initial_balance", C.c_double),
        ("monthly_contribution", C.c_double),
        ("monthly_expenses", C.c_double),
        ("monthly_amount_today", C.c_double),
        ("start_at_age", C.c_double),
        ("duration_years", C.c_int32),
        ("reserved", C.c_int32),
    ]


class McrOptionOutcomes(C.Structure):
    """mcr_option_outcomes: the row slabs of the ``*_outcomes_rng`` probes (device pointers; None = not requested)."""

    _fields_ = [
        ("final_balance", C.c_void_p),
        ("years_to_ruin", C.c_void_p),
        ("path_stride", C.c_int64),
    ]


class McrSpendingRule(C.Structure):
    """mcr_spending_rule: the withdrawal-rate guardrail of include/mcr.h."""

    _fields_ = [
        ("upper", C.c_double),
        ("lower", C.c_double),
        ("cut", C.c_double),
        ("raise", C.c_double),
        ("floor", C.c_double),
        ("ceiling", C.c_double),
    ]


class McrRuleOutputs(C.Structure):
    """mcr_rule_outputs: the per-year counts and the optional multiplier rows of mcr_run_rule_rng (device pointers)."""

    _fields_ = [
        ("year_counts", C.c_void_p),
        ("multipliers", C.c_void_p),
        ("path_stride", C.c_int64),
    ]


class McrRuleOption(C.Structure):
    """One record of a rule probe (include/mcr.h: mcr_rule_option): the three scenario levers and the option's spending rule."""

    _fields_ = [
        ("initial_balance", C.c_double),
        ("monthly_contribution", C.c_double),
        ("monthly_expenses", C.c_double),
        ("rule", McrSpendingRule),
    ]


class McrAllocationOption(C.Structure):
    """One record of an allocation probe (include/mcr.h: mcr_allocation_option): the three scenario levers and the share of
    the first asset."""

    _fields_ = [
        ("initial_balance", C.c_double),
        ("monthly_contribution", C.c_double),
        ("monthly_expenses", C.c_double),
        ("allocation_inv1_pct", C.c_double),
    ]


class McrGlideOption(C.Structure):
    """One record of a glide probe (include/mcr.h: mcr_glide_option): the three scenario levers and the option's table, entries
    ``first_weight .. first_weight + n_weights`` of the call's flat array of weights."""

    _fields_ = [
        ("initial_balance", C.c_double),
        ("monthly_contribution", C.c_double),
        ("monthly_expenses", C.c_double),
        ("first_weight", C.c_int32),
        ("n_weights", C.c_int32),
    ]


class McrSizes(C.Structure):
    _fields_ = [
        ("total_months", C.c_int32),
        ("shock_rows", C.c_int32),
        ("num_working_years", C.c_int32),
        ("trajectory_len", C.c_int32),
        ("retirement_years", C.c_int32),
        ("ruin_bins", C.c_int32),
    ]


class McrOutputs(C.Structure):
    """Pointers are plain addresses (device or host, depending on the entry point)."""

    _fields_ = [
        ("start_balance", C.c_void_p),
        ("final_balance", C.c_void_p),
        ("years_to_ruin", C.c_void_p),
        ("first_year_gross_withdrawal", C.c_void_p),
        ("first_year_real_gross_withdrawal", C.c_void_p),
        ("inflation_at_retirement", C.c_void_p),
        ("success", C.c_void_p),
        ("trajectory", C.c_void_p),
        ("real_trajectory", C.c_void_p),
        ("withdrawal_rate_trajectory", C.c_void_p),
        ("path_stride", C.c_int64),
        ("counters", C.c_void_p),
        ("wr_obs_counts", C.c_void_p),
        ("ruin_year_bins", C.c_void_p),
        ("hist_edges", C.c_void_p),
        ("hist_bins", C.c_void_p),
        ("hist_n_bins", C.c_int32),
        ("hist_reserved", C.c_int32),
    ]


class McrYearBins(C.Structure):
    """Edges and tables of a yearly-bins launch (include/mcr.h: mcr_year_bins); addresses like McrOutputs."""

    _fields_ = [
        ("edges", C.c_void_p),
        ("n_bins", C.c_int32),
        ("wr_edges", C.c_void_p),
        ("n_wr_bins", C.c_int32),
        ("trajectory_bins", C.c_void_p),
        ("real_trajectory_bins", C.c_void_p),
        ("wr_bins", C.c_void_p),
        ("final_success_bins", C.c_void_p),
    ]


class McrRuleYearBins(C.Structure):
    """The rule's tables of a yearly-bins launch under a spending rule (include/mcr.h: mcr_rule_year_bins); addresses like McrOutputs."""

    _fields_ = [
        ("m_edges", C.c_void_p),
        ("n_m_bins", C.c_int32),
        ("multiplier_bins", C.c_void_p),
        ("year_counts", C.c_void_p),
    ]


#: The symbols include/mcr.h declares; tests check that the built library exports them all.
ABI_SYMBOLS = (
    "mcr_abi_version",
    "mcr_device_count",
    "mcr_last_error",
    "mcr_query_sizes",
    "mcr_stream_start_month_index",
    "mcr_k1_growth_form",
    "mcr_k1_month_form",
    "mcr_k1_stream_form",
    "mcr_k1_screen",
    "mcr_screen_paths_rng",
    "mcr_k1_kept_streams",
    "mcr_run_batch",
    "mcr_run_batch_host",
    "mcr_draw_shocks_host",
    "mcr_run_batch_rng",
    "mcr_run_batch_host_rng",
    "mcr_draw_shocks_host_rng",
    "mcr_probe_months_rng",
    "mcr_probe_expenses_rng",
    "mcr_probe_contributions_rng",
    "mcr_probe_scenarios_rng",
    "mcr_probe_assumptions_rng",
    "mcr_probe_assumptions_last_fanout_launches",
    "mcr_probe_income_rng",
    "mcr_probe_income_last_fanout_launches",
    "mcr_joint_mask_words",
    "mcr_probe_scenarios_joint_rng",
    "mcr_probe_assumptions_joint_rng",
    "mcr_probe_income_joint_rng",
    "mcr_joint_counts",
    "mcr_probe_scenarios_outcomes_rng",
    "mcr_probe_assumptions_outcomes_rng",
    "mcr_probe_income_outcomes_rng",
    "mcr_ruin_month_counts",
    "mcr_probe_grid_rng",
    "mcr_run_batch_multi_host_rng",
    "mcr_run_year_bins_rng",
    "mcr_run_year_bins_host_rng",
    "mcr_run_year_bins_multi_host_rng",
    "mcr_validate_params",
    "mcr_validate_spending_rule",
    "mcr_run_rule_rng",
    "mcr_run_rule_year_bins_rng",
    "mcr_run_rule_year_bins_host_rng",
    "mcr_probe_rules_rng",
    "mcr_probe_rules_joint_rng",
    "mcr_probe_rules_outcomes_rng",
    "mcr_probe_rules_last_fanout_launches",
    "mcr_probe_rule_grid_rng",
    "mcr_probe_rule_grid_last_fanout_launches",
    "mcr_probe_allocations_rng",
    "mcr_probe_allocations_joint_rng",
    "mcr_probe_allocations_outcomes_rng",
    "mcr_probe_allocations_last_fanout_launches",
    "mcr_probe_glide_paths_rng",
    "mcr_probe_glide_paths_joint_rng",
    "mcr_probe_glide_paths_outcomes_rng",
    "mcr_probe_glide_paths_last_fanout_launches",
    "mcr_run_glide_rng",
    "mcr_run_glide_year_bins_rng",
    "mcr_run_glide_year_bins_host_rng",
    "mcr_release_cached",
    "mcr_sample_columns",
    "mcr_eval_helper_host",
    "mcr_row_quantiles_scratch_bytes",
    "mcr_row_quantiles",
    "mcr_row_quantiles_last_fallback_rows",
    "mcr_row_quantiles_sharded",
    "mcr_row_quantiles_reduce_block",
    "mcr_row_quantiles_begin",
    "mcr_row_quantiles_hist",
    "mcr_row_quantiles_scan",
    "mcr_minmax_success",
    "mcr_histogram_success",
    "mcr_summary_stat_rows",
)

_LIB_NAME = "libmcr_hip.so"
_lib: Optional[C.CDLL] = None
_lib_lock = threading.Lock()


def library_path() -> str:
    """csrc/libmcr_hip.so next to this file; MCR_HIP_LIBRARY names another build of the same ABI (A/B measurements of
    compile-time variants, tools/)."""
    return os.environ.get("MCR_HIP_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", _LIB_NAME)


def _declare(lib: C.CDLL) -> None:
    P = C.POINTER
    lib.mcr_abi_version.restype = C.c_int
    lib.mcr_abi_version.argtypes = []
    lib.mcr_device_count.restype = C.c_int
    lib.mcr_device_count.argtypes = []
    lib.mcr_last_error.restype = C.c_char_p
    lib.mcr_last_error.argtypes = []
    lib.mcr_query_sizes.restype = C.c_int
    lib.mcr_query_sizes.argtypes = [P(McrParams), C.c_int32, P(McrSizes)]
    lib.mcr_stream_start_month_index.restype = C.c_int32
    lib.mcr_stream_start_month_index.argtypes = [C.c_double, C.c_int32, C.c_double]
    lib.mcr_k1_growth_form.restype = C.c_int
    lib.mcr_k1_growth_form.argtypes = [P(McrParams), C.c_int32, P(C.c_int32)]
    if hasattr(lib, "mcr_k1_month_form"):   # (an MCR_HIP_LIBRARY built from an earlier tree, for A/B runs, has neither)
        lib.mcr_k1_month_form.restype = C.c_int
        lib.mcr_k1_month_form.argtypes = [P(McrParams), C.c_int32, P(C.c_int32)]
        lib.mcr_k1_kept_streams.restype = C.c_int
        lib.mcr_k1_kept_streams.argtypes = [P(McrParams), C.c_int32, P(C.c_int32), P(C.c_int32), C.c_int32, P(C.c_int32)]
    if hasattr(lib, "mcr_k1_stream_form"):  # (likewise)
        lib.mcr_k1_stream_form.restype = C.c_int
        lib.mcr_k1_stream_form.argtypes = [P(McrParams), C.c_int32, P(C.c_int32)]
    if hasattr(lib, "mcr_k1_screen"):       # (likewise)
        lib.mcr_k1_screen.restype = C.c_int
        lib.mcr_k1_screen.argtypes = [P(McrParams), P(McrRng), C.c_int32, C.c_uint64, C.c_int32, P(C.c_int32)]
        lib.mcr_screen_paths_rng.restype = C.c_int
        lib.mcr_screen_paths_rng.argtypes = [P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.mcr_run_batch.restype = C.c_int
    lib.mcr_run_batch.argtypes = [
        P(McrParams), C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32,
        C.c_void_p, P(McrOutputs), C.c_int, C.c_void_p,
    ]
    lib.mcr_run_batch_host.restype = C.c_int
    lib.mcr_run_batch_host.argtypes = [
        P(McrParams), C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32,
        C.c_void_p, P(McrOutputs), C.c_int,
    ]
    lib.mcr_draw_shocks_host.restype = C.c_int
    lib.mcr_draw_shocks_host.argtypes = [
        C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, C.c_double,
        C.c_void_p, C.c_int,
    ]
    lib.mcr_run_batch_rng.restype = C.c_int
    lib.mcr_run_batch_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32,
        C.c_void_p, P(McrOutputs), C.c_int, C.c_void_p,
    ]
    lib.mcr_probe_months_rng.restype = C.c_int
    lib.mcr_probe_months_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, P(C.c_int32), C.c_int32,
        C.c_void_p, C.c_int, C.c_void_p,
    ]
    lib.mcr_probe_expenses_rng.restype = C.c_int
    lib.mcr_probe_expenses_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(C.c_double), C.c_int32,
        C.c_void_p, C.c_int, C.c_void_p,
    ]
    lib.mcr_probe_contributions_rng.restype = C.c_int
    lib.mcr_probe_contributions_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(C.c_double), C.c_int32,
        C.c_void_p, C.c_int, C.c_void_p,
    ]
    if hasattr(lib, "mcr_probe_scenarios_rng"):   # (an MCR_HIP_LIBRARY built from an earlier tree, for A/B runs, lacks it)
        lib.mcr_probe_scenarios_rng.restype = C.c_int
        lib.mcr_probe_scenarios_rng.argtypes = [
            P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(McrScenario), C.c_int32,
            C.c_void_p, C.c_int, C.c_void_p,
        ]
    if hasattr(lib, "mcr_probe_assumptions_rng"):   # (likewise)
        lib.mcr_probe_assumptions_rng.restype = C.c_int
        lib.mcr_probe_assumptions_rng.argtypes = [
            P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(McrAssumptions), C.c_int32,
            C.c_void_p, C.c_int, C.c_void_p,
        ]
        lib.mcr_probe_assumptions_last_fanout_launches.restype = C.c_int
        lib.mcr_probe_assumptions_last_fanout_launches.argtypes = []
    if hasattr(lib, "mcr_probe_income_rng"):   # (likewise)
        lib.mcr_probe_income_rng.restype = C.c_int
        lib.mcr_probe_income_rng.argtypes = [
            P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, P(McrIncomeOption), C.c_int32,
            C.c_void_p, C.c_int, C.c_void_p,
        ]
        lib.mcr_probe_income_last_fanout_launches.restype = C.c_int
        lib.mcr_probe_income_last_fanout_launches.argtypes = []
    if hasattr(lib, "mcr_joint_counts"):   # (likewise)
        lib.mcr_joint_mask_words.restype = C.c_uint64
        lib.mcr_joint_mask_words.argtypes = [C.c_uint64]
        joint_out = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]   # counts, masks, joint, extremes, device, stream
        head = [P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32]
        lib.mcr_probe_scenarios_joint_rng.restype = C.c_int
        lib.mcr_probe_scenarios_joint_rng.argtypes = head + [P(McrScenario), C.c_int32] + joint_out
        lib.mcr_probe_assumptions_joint_rng.restype = C.c_int
        lib.mcr_probe_assumptions_joint_rng.argtypes = head + [P(McrAssumptions), C.c_int32] + joint_out
        lib.mcr_probe_income_joint_rng.restype = C.c_int
        lib.mcr_probe_income_joint_rng.argtypes = head + [C.c_int32, P(McrIncomeOption), C.c_int32] + joint_out
        lib.mcr_joint_counts.restype = C.c_int
        lib.mcr_joint_counts.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(lib, "mcr_ruin_month_counts"):   # (likewise)
        out = [C.c_void_p, P(McrOptionOutcomes), C.c_int, C.c_void_p]   # counts, rows, device, stream
        head = [P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32]
        lib.mcr_probe_scenarios_outcomes_rng.restype = C.c_int
        lib.mcr_probe_scenarios_outcomes_rng.argtypes = head + [P(McrScenario), C.c_int32] + out
        lib.mcr_probe_assumptions_outcomes_rng.restype = C.c_int
        lib.mcr_probe_assumptions_outcomes_rng.argtypes = head + [P(McrAssumptions), C.c_int32] + out
        lib.mcr_probe_income_outcomes_rng.restype = C.c_int
        lib.mcr_probe_income_outcomes_rng.argtypes = head + [C.c_int32, P(McrIncomeOption), C.c_int32] + out
        lib.mcr_ruin_month_counts.restype = C.c_int
        lib.mcr_ruin_month_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    lib.mcr_probe_grid_rng.restype = C.c_int
    lib.mcr_probe_grid_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, P(C.c_int32), C.c_int32, P(C.c_double), C.c_int32,
        C.c_void_p, C.c_int, C.c_void_p,
    ]
    lib.mcr_run_batch_host_rng.restype = C.c_int
    lib.mcr_run_batch_host_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32,
        C.c_void_p, P(McrOutputs), C.c_int,
    ]
    lib.mcr_run_batch_multi_host_rng.restype = C.c_int
    lib.mcr_run_batch_multi_host_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32,
        C.c_void_p, P(McrOutputs), P(C.c_int32), C.c_int32,
    ]
    lib.mcr_run_year_bins_rng.restype = C.c_int
    lib.mcr_run_year_bins_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(McrOutputs), P(McrYearBins), C.c_int, C.c_void_p,
    ]
    lib.mcr_run_year_bins_host_rng.restype = C.c_int
    lib.mcr_run_year_bins_host_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(McrOutputs), P(McrYearBins), C.c_int,
    ]
    lib.mcr_run_year_bins_multi_host_rng.restype = C.c_int
    lib.mcr_run_year_bins_multi_host_rng.argtypes = [
        P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(McrOutputs), P(McrYearBins), P(C.c_int32), C.c_int32,
    ]
    lib.mcr_validate_params.restype = C.c_int
    lib.mcr_validate_params.argtypes = [P(McrParams)]
    if hasattr(lib, "mcr_run_rule_rng"):   # (an MCR_HIP_LIBRARY built from an earlier tree, for A/B runs, lacks it)
        lib.mcr_validate_spending_rule.restype = C.c_int
        lib.mcr_validate_spending_rule.argtypes = [P(McrSpendingRule)]
        lib.mcr_run_rule_rng.restype = C.c_int
        lib.mcr_run_rule_rng.argtypes = [
            P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(McrSpendingRule), P(McrOutputs),
            P(McrRuleOutputs), C.c_int, C.c_void_p,
        ]
    if hasattr(lib, "mcr_run_rule_year_bins_rng"):   # (likewise)
        head = [P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(McrSpendingRule), P(McrOutputs),
                P(McrYearBins), P(McrRuleYearBins)]
        lib.mcr_run_rule_year_bins_rng.restype = C.c_int
        lib.mcr_run_rule_year_bins_rng.argtypes = head + [C.c_int, C.c_void_p]
        lib.mcr_run_rule_year_bins_host_rng.restype = C.c_int
        lib.mcr_run_rule_year_bins_host_rng.argtypes = head + [C.c_int]
    if hasattr(lib, "mcr_probe_rules_rng"):   # (likewise)
        head = [P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(McrRuleOption), C.c_int32,
                C.c_void_p, C.c_void_p]   # ..., options, n_options, counts, year_counts
        lib.mcr_probe_rules_rng.restype = C.c_int
        lib.mcr_probe_rules_rng.argtypes = head + [C.c_int, C.c_void_p]
        lib.mcr_probe_rules_joint_rng.restype = C.c_int
        lib.mcr_probe_rules_joint_rng.argtypes = head + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]   # masks, joint, extremes
        lib.mcr_probe_rules_outcomes_rng.restype = C.c_int
        lib.mcr_probe_rules_outcomes_rng.argtypes = head + [P(McrOptionOutcomes), C.c_int, C.c_void_p]
        lib.mcr_probe_rules_last_fanout_launches.restype = C.c_int
        lib.mcr_probe_rules_last_fanout_launches.argtypes = []
    if hasattr(lib, "mcr_probe_allocations_rng"):   # (likewise)
        head = [P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(McrAllocationOption), C.c_int32,
                C.c_void_p]       # ..., options, n_options, counts
        lib.mcr_probe_allocations_rng.restype = C.c_int
        lib.mcr_probe_allocations_rng.argtypes = head + [C.c_int, C.c_void_p]
        lib.mcr_probe_allocations_joint_rng.restype = C.c_int
        lib.mcr_probe_allocations_joint_rng.argtypes = head + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]   # masks, joint, extremes
        lib.mcr_probe_allocations_outcomes_rng.restype = C.c_int
        lib.mcr_probe_allocations_outcomes_rng.argtypes = head + [P(McrOptionOutcomes), C.c_int, C.c_void_p]
        lib.mcr_probe_allocations_last_fanout_launches.restype = C.c_int
        lib.mcr_probe_allocations_last_fanout_launches.argtypes = []
    if hasattr(lib, "mcr_probe_glide_paths_rng"):   # (likewise)
        head = [P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(C.c_double), C.c_int32, P(McrGlideOption),
                C.c_int32, C.c_void_p]       # ..., weights, n_weights, options, n_options, counts
        lib.mcr_probe_glide_paths_rng.restype = C.c_int
        lib.mcr_probe_glide_paths_rng.argtypes = head + [C.c_int, C.c_void_p]
        lib.mcr_probe_glide_paths_joint_rng.restype = C.c_int
        lib.mcr_probe_glide_paths_joint_rng.argtypes = head + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]   # masks, joint, extremes
        lib.mcr_probe_glide_paths_outcomes_rng.restype = C.c_int
        lib.mcr_probe_glide_paths_outcomes_rng.argtypes = head + [P(McrOptionOutcomes), C.c_int, C.c_void_p]
        lib.mcr_probe_glide_paths_last_fanout_launches.restype = C.c_int
        lib.mcr_probe_glide_paths_last_fanout_launches.argtypes = []
    if hasattr(lib, "mcr_run_glide_rng"):   # (likewise)
        head = [P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, P(C.c_double), C.c_int32, P(McrOutputs)]   # ..., weights, n_weights, out
        lib.mcr_run_glide_rng.restype = C.c_int
        lib.mcr_run_glide_rng.argtypes = head + [C.c_int, C.c_void_p]
        lib.mcr_run_glide_year_bins_rng.restype = C.c_int
        lib.mcr_run_glide_year_bins_rng.argtypes = head + [P(McrYearBins), C.c_int, C.c_void_p]
        lib.mcr_run_glide_year_bins_host_rng.restype = C.c_int
        lib.mcr_run_glide_year_bins_host_rng.argtypes = head + [P(McrYearBins), C.c_int]
    if hasattr(lib, "mcr_probe_rule_grid_rng"):   # (likewise)
        lib.mcr_probe_rule_grid_rng.restype = C.c_int
        lib.mcr_probe_rule_grid_rng.argtypes = [
            P(McrParams), P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, P(C.c_int32), C.c_int32, P(C.c_double), C.c_int32,
            P(McrSpendingRule), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,   # ..., rule, counts, year_counts
        ]
        lib.mcr_probe_rule_grid_last_fanout_launches.restype = C.c_int
        lib.mcr_probe_rule_grid_last_fanout_launches.argtypes = []
    lib.mcr_release_cached.restype = C.c_int
    lib.mcr_release_cached.argtypes = [C.c_int]
    lib.mcr_sample_columns.restype = C.c_int
    lib.mcr_sample_columns.argtypes = [C.c_uint32, C.c_uint64, C.c_int32, C.c_void_p]
    lib.mcr_draw_shocks_host_rng.restype = C.c_int
    lib.mcr_draw_shocks_host_rng.argtypes = [
        P(McrRng), C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, C.c_double, C.c_void_p, C.c_int,
    ]
    lib.mcr_eval_helper_host.restype = C.c_int
    lib.mcr_eval_helper_host.argtypes = [
        C.c_int, P(McrParams), C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
    ]
    lib.mcr_row_quantiles_scratch_bytes.restype = C.c_int64
    lib.mcr_row_quantiles_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int64]
    lib.mcr_row_quantiles.restype = C.c_int
    lib.mcr_row_quantiles.argtypes = [
        C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
    ]
    lib.mcr_row_quantiles_sharded.restype = C.c_int
    lib.mcr_row_quantiles_sharded.argtypes = [
        C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_int32, C.c_int32, REDUCE_FN, C.c_void_p, C.c_int, C.c_void_p,
    ]
    lib.mcr_row_quantiles_reduce_block.restype = C.c_int64
    lib.mcr_row_quantiles_reduce_block.argtypes = [C.c_int32, P(C.c_int64)]
    lib.mcr_row_quantiles_begin.restype = C.c_int
    lib.mcr_row_quantiles_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_void_p]
    lib.mcr_row_quantiles_hist.restype = C.c_int
    lib.mcr_row_quantiles_hist.argtypes = [
        C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int, C.c_void_p,
    ]
    lib.mcr_row_quantiles_scan.restype = C.c_int
    lib.mcr_row_quantiles_scan.argtypes = [
        C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
    ]
    lib.mcr_minmax_success.restype = C.c_int
    lib.mcr_minmax_success.argtypes = [
        C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
    ]
    lib.mcr_histogram_success.restype = C.c_int
    lib.mcr_histogram_success.argtypes = [
        C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
        C.c_int, C.c_void_p,
    ]
    lib.mcr_row_quantiles_last_fallback_rows.restype = C.c_int
    lib.mcr_row_quantiles_last_fallback_rows.argtypes = []
    lib.mcr_summary_stat_rows.restype = C.c_int
    lib.mcr_summary_stat_rows.argtypes = [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
    ]


def load_library() -> C.CDLL:
    """Load (once) and return the HIP engine.  Raises RuntimeError if it is not built."""
    global _lib
    with _lib_lock:
        if _lib is None:
            path = library_path()
            if not os.path.exists(path):
                raise RuntimeError(
                    f"HIP engine not built: {path} is missing. Run "
                    "`python -c 'import __graft_entry__ as g; g.build()'` "
                    "(there is no CPU fallback)."
                )
            # One HIP runtime per process: PyTorch (our device-memory / stream / RCCL plumbing) ships
            # its own libamdhip64 and looks it up by a different file name than its SONAME, so if
            # this library pulled in the system runtime first, torch would load a second copy and
            # find "No HIP GPUs".  Importing torch first makes both bind to the same runtime.
            try:
                import torch  # noqa: F401
            except Exception:  # torch-less callers (plain ctypes integration) use the system runtime
                pass
            try:
                lib = C.CDLL(path)
            except OSError as exc:
                raise RuntimeError(f"cannot load HIP engine {path}: {exc}") from exc
            _declare(lib)
            if lib.mcr_abi_version() != MCR_ABI_VERSION:
                raise RuntimeError(
                    f"{path}: ABI version {lib.mcr_abi_version()} != {MCR_ABI_VERSION}; rebuild"
                )
            _lib = lib
        return _lib


def last_error() -> str:
    msg = load_library().mcr_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {last_error()}")


def device_count() -> int:
    return int(load_library().mcr_device_count())


def require_device() -> None:
    if device_count() <= 0:
        raise RuntimeError(
            "no usable HIP device: the Monte Carlo path engine runs only on a gfx950 GPU "
            "(there is no CPU fallback)"
        )


def helper_arity(which: int):
    return _HELPER_ARITY[which]
