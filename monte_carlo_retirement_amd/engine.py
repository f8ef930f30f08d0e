"""Python face of the C ABI (include/mcr.h): numpy in / numpy out, HIP underneath.

Everything here runs the hand-written gfx950 kernels in csrc/ — there is no CPU path.
Two families:

* ``*_host`` helpers move small batches through host (numpy) buffers; the library
  allocates device scratch, launches, copies back (``mcr_run_batch_host``).
* :class:`DeviceBatch` keeps the outputs of a large batch resident in HBM (torch tensors
  are used purely as device-memory handles / stream plumbing) for the aggregation kernels.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import _native as N
from ._native import McrAssumptions, McrIncomeOption, McrOptionOutcomes, McrOutputs, McrParams, McrRng, McrScenario, McrSizes, McrYearBins, McrRuleYearBins

SUMMARY_FIELDS = (
    "start_balance",
    "final_balance",
    "years_to_ruin",
    "first_year_gross_withdrawal",
    "first_year_real_gross_withdrawal",
    "inflation_at_retirement",
)


def query_sizes(params: McrParams, working_months: int) -> McrSizes:
    """Shapes for (params, working_months); ``ValueError`` on invalid input."""
    sz = McrSizes()
    rc = N.load_library().mcr_query_sizes(C.byref(params), int(working_months), C.byref(sz))
    if rc != 0:
        raise ValueError(N.last_error() or "invalid params / working_months")
    return sz


def growth_form(params: McrParams, working_months: int) -> int:
    """Growth form (0, 1 or 3) a whole-path count-only launch of these parameters runs (mcr_k1_growth_form; honours
    MCR_K1_GROWTH_FORM); ``ValueError`` if the parameters, or a forced form they do not qualify for, are invalid."""
    mask = C.c_int32(-1)
    rc = N.load_library().mcr_k1_growth_form(C.byref(params), int(working_months), C.byref(mask))
    if rc != 0:
        raise ValueError(N.last_error() or "invalid params / growth form")
    return int(mask.value)


def month_form(params: McrParams, working_months: int) -> int:
    """Month form (0 or 1) a whole-path count-only launch of these parameters runs (mcr_k1_month_form; honours
    MCR_K1_MONTH_FORM); ``ValueError`` if the parameters, or a forced form they do not qualify for, are invalid."""
    mask = C.c_int32(-1)
    rc = N.load_library().mcr_k1_month_form(C.byref(params), int(working_months), C.byref(mask))
    if rc != 0:
        raise ValueError(N.last_error() or "invalid params / month form")
    return int(mask.value)


def stream_form(params: McrParams, working_months: int) -> int:
    """Stream form (0 or 1) a whole-path count-only launch of these parameters runs (mcr_k1_stream_form; honours
    MCR_K1_STREAM_FORM); ``ValueError`` if the parameters, or a forced form they do not qualify for, are invalid."""
    mask = C.c_int32(-1)
    rc = N.load_library().mcr_k1_stream_form(C.byref(params), int(working_months), C.byref(mask))
    if rc != 0:
        raise ValueError(N.last_error() or "invalid params / stream form")
    return int(mask.value)


def screen(params: McrParams, working_months: int, n_paths: int, rng: Optional[McrRng] = None, hist_n_bins: int = 0) -> bool:
    """Whether a count-only launch of ``n_paths`` paths takes the screened route (mcr_k1_screen; honours MCR_K1_SCREEN,
    MCR_K1_SCREEN_MIN_PATHS and the knobs that address the classic kernels).  ``rng``: a descriptor, or None for the
    engine's own stream; ``ValueError`` if the parameters or a knob's value are invalid."""
    out = C.c_int32(-1)
    rc = N.load_library().mcr_k1_screen(C.byref(params), C.byref(rng) if rng is not None else None, int(working_months),
                                        int(n_paths), int(hist_n_bins), C.byref(out))
    if rc != 0:
        raise ValueError(N.last_error() or "invalid params / screen knob")
    return bool(out.value)


def screen_paths(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                 device: int = 0) -> Dict[str, np.ndarray]:
    """The screening kernel alone (mcr_screen_paths_rng; tests and tools): per path ``cls`` (0 safe, 1 doubtful), ``min_ratio``
    (lowest capacity / need seen) and ``final_total`` (b1 + b2 where the lane stopped), all in the kernel's fp32."""
    N.require_device()
    n = int(n_paths)
    res = {"cls": np.empty(n, dtype=np.uint8), "min_ratio": np.empty(n, dtype=np.float32), "final_total": np.empty(n, dtype=np.float32)}
    rng = _as_rng(seed)
    rc = N.load_library().mcr_screen_paths_rng(C.byref(params), C.byref(rng), int(stream_id), int(path_begin), n, int(working_months),
                                               res["cls"].ctypes.data, res["min_ratio"].ctypes.data, res["final_total"].ctypes.data, int(device))
    if rc != 0:
        raise RuntimeError(N.last_error() or f"mcr_screen_paths_rng failed ({rc})")
    return res


def kept_streams(params: McrParams, working_months: int) -> list:
    """``(index, lock_slot)`` of every ``other_income_streams`` record the path kernel is given, in list order
    (mcr_k1_kept_streams): records that pay nothing are left out, and the lock slots (-1: an indexed stream has none) are
    numbered over the kept ones."""
    cap = max(int(params.n_streams), 1)
    index, slot, n = (C.c_int32 * cap)(), (C.c_int32 * cap)(), C.c_int32(-1)
    rc = N.load_library().mcr_k1_kept_streams(C.byref(params), int(working_months), index, slot, cap, C.byref(n))
    if rc != 0:
        raise ValueError(N.last_error() or "invalid params")
    return [(int(index[i]), int(slot[i])) for i in range(n.value)]


def stream_start_month_index(current_age: float, working_months: int, start_at_age: float) -> int:
    return int(N.load_library().mcr_stream_start_month_index(current_age, working_months, start_at_age))


def _as_rng(seed, device: Optional[int] = None) -> McrRng:
    """`seed` may be an int (Philox key) or a ready McrRng descriptor (copied: callers' objects are never mutated).

    ``device``: the HIP ordinal of an entry point that takes DEVICE pointers.  A history descriptor
    (``_native.history_rng``) points at host memory; its copy then points at a device copy of the table, made once per
    device and kept with the caller's descriptor."""
    if isinstance(seed, McrRng):
        dup = McrRng()
        C.memmove(C.byref(dup), C.byref(seed), C.sizeof(McrRng))
        table = getattr(seed, "_history_table", None)
        dup._history_table = table          # (the copy keeps what it points at alive)
        if device is not None and seed.kind == N.MCR_RNG_HISTORY:
            if table is None:
                raise ValueError("history rng: build the descriptor with _native.history_rng (it owns the table)")
            import torch

            cache = seed.__dict__.setdefault("_history_device", {})
            if int(device) not in cache:
                cache[int(device)] = torch.as_tensor(np.array(table), device=torch.device("cuda", int(device)))   # (a copy: the table is read-only)
            dup._history_device = cache[int(device)]
            dup.history = dup._history_device.data_ptr()
        return dup
    return N.philox_rng(int(seed))


def hist_edge_array(edges) -> np.ndarray:
    """Bin edges of the in-kernel final-balance histogram as the contiguous float64 array the ABI wants;
    ``ValueError`` unless they are finite, ascending and 2..MCR_MAX_HIST_BINS+1 long (np.histogram's own rule)."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
    if not (2 <= e.shape[0] <= N.MCR_MAX_HIST_BINS + 1):
        raise ValueError(f"hist_edges: need 2..{N.MCR_MAX_HIST_BINS + 1} edges, got {e.shape[0]}")
    if not np.all(np.isfinite(e)) or np.any(e[1:] < e[:-1]):
        raise ValueError("hist_edges must be finite and increase monotonically")
    return e


def uniform_hist_edges(value_range, n_bins: int) -> np.ndarray:
    """The edges ``np.histogram(x, bins=n_bins, range=value_range)`` bins on (numpy/lib/_histograms_impl.py:
    ``_get_outer_edges`` widens a degenerate range by 0.5 either side, then ``np.linspace``)."""
    lo, hi = (float(v) for v in value_range)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        raise ValueError("value_range must be finite with lo <= hi")
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, int(n_bins) + 1, endpoint=True, dtype=np.float64)


def run_batch_host(
    params: McrParams,
    seed,
    stream_id: int,
    path_begin: int,
    n_paths: int,
    working_months: int,
    injected_shocks: Optional[np.ndarray] = None,
    want_summary: bool = True,
    want_trajectories: bool = True,
    want_bins: bool = True,
    device: int = 0,
    path_seeds: Optional[np.ndarray] = None,
    devices: Optional[Sequence[int]] = None,
    hist_edges: Optional[np.ndarray] = None,
) -> Dict[str, np.ndarray]:
    """Simulate paths [path_begin, path_begin+n_paths) on the GPU; numpy arrays out.

    ``device``: HIP ordinal, or ``_native.MCR_DEVICE_ALL`` = shard over every visible device.  ``devices``: an
    explicit device list instead (``mcr_run_batch_multi_host_rng``: one host thread per entry, contiguous shards
    of the path range, counters summed on the host) — same numbers whatever the list.

    ``seed``: int (Philox key) or an ``McrRng`` (e.g. ``_native.numpy_rng(main_seed, child_offset)``);
    ``path_seeds``: explicit uint32 seed per path for the NumPy stream.

    Keys follow ``mcr_outputs``: the six float summary fields + ``success`` (uint8),
    ``trajectory``/``real_trajectory`` ``[T, n]``, ``withdrawal_rate_trajectory`` ``[ry, n]``,
    ``counters`` ``[2]``, ``wr_obs_counts`` ``[ry]``, ``ruin_year_bins`` ``[ry+2]``.

    ``hist_edges``: ascending bin edges ``[n_bins + 1]`` -> ``hist_bins`` ``[n_bins]`` =
    ``np.histogram(final_balance[success], bins=hist_edges)[0]``, binned inside the path kernel
    (``mcr_outputs.hist_bins``; no per-path output is needed for it).
    """
    lib = N.load_library()
    N.require_device()
    sz = query_sizes(params, working_months)
    n = int(n_paths)
    res: Dict[str, np.ndarray] = {}
    o = McrOutputs()
    o.path_stride = n
    if want_summary:
        for k in SUMMARY_FIELDS:
            res[k] = np.empty(n, dtype=np.float64)
            setattr(o, k, res[k].ctypes.data)
        res["success"] = np.empty(n, dtype=np.uint8)
        o.success = res["success"].ctypes.data
    if want_trajectories:
        res["trajectory"] = np.empty((sz.trajectory_len, n), dtype=np.float64)
        res["real_trajectory"] = np.empty((sz.trajectory_len, n), dtype=np.float64)
        res["withdrawal_rate_trajectory"] = np.empty((sz.retirement_years, n), dtype=np.float64)
        o.trajectory = res["trajectory"].ctypes.data
        o.real_trajectory = res["real_trajectory"].ctypes.data
        o.withdrawal_rate_trajectory = res["withdrawal_rate_trajectory"].ctypes.data
    res["counters"] = np.zeros(N.MCR_N_COUNTERS, dtype=np.uint64)
    o.counters = res["counters"].ctypes.data
    if want_bins:
        res["wr_obs_counts"] = np.zeros(sz.retirement_years, dtype=np.uint64)
        res["ruin_year_bins"] = np.zeros(sz.ruin_bins, dtype=np.uint64)
        o.wr_obs_counts = res["wr_obs_counts"].ctypes.data
        o.ruin_year_bins = res["ruin_year_bins"].ctypes.data
    edges_arr = None
    if hist_edges is not None:
        edges_arr = hist_edge_array(hist_edges)
        res["hist_bins"] = np.zeros(edges_arr.shape[0] - 1, dtype=np.uint64)
        o.hist_edges = edges_arr.ctypes.data
        o.hist_bins = res["hist_bins"].ctypes.data
        o.hist_n_bins = edges_arr.shape[0] - 1
    inj = None
    inj_arr = None
    if injected_shocks is not None:
        inj_arr = np.ascontiguousarray(injected_shocks, dtype=np.float64)
        if inj_arr.shape != (n, sz.shock_rows, 3):
            raise ValueError(f"injected_shocks shape {inj_arr.shape} != {(n, sz.shock_rows, 3)}")
        inj = inj_arr.ctypes.data
    rng = _as_rng(seed)
    seeds_arr = None
    if path_seeds is not None:
        seeds_arr = np.ascontiguousarray(path_seeds, dtype=np.uint32)
        if seeds_arr.shape != (n,):
            raise ValueError("path_seeds must have one uint32 per path")
        rng.path_seeds = seeds_arr.ctypes.data
    if devices is not None:
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        rc = lib.mcr_run_batch_multi_host_rng(
            C.byref(params), C.byref(rng), int(stream_id), int(path_begin), n, int(working_months),
            inj, C.byref(o), devs, len(devices),
        )
        N.check(rc, "mcr_run_batch_multi_host_rng")
        return res
    rc = lib.mcr_run_batch_host_rng(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), n, int(working_months),
        inj, C.byref(o), int(device),
    )
    N.check(rc, "mcr_run_batch_host_rng")
    return res


def draw_shocks_host(
    seed, stream_id: int, path_begin: int, n_paths: int, n_months: int, rho: float, device: int = 0,
    path_seeds: Optional[np.ndarray] = None,
) -> np.ndarray:
    """Engine shock rows ``[n_paths, n_months, 3]`` (equity, inflation, premium) from the GPU."""
    N.require_device()
    out = np.empty((int(n_paths), int(n_months), 3), dtype=np.float64)
    rng = _as_rng(seed)
    seeds_arr = None
    if path_seeds is not None:
        seeds_arr = np.ascontiguousarray(path_seeds, dtype=np.uint32)
        rng.path_seeds = seeds_arr.ctypes.data
    rc = N.load_library().mcr_draw_shocks_host_rng(
        C.byref(rng), int(stream_id), int(path_begin), int(n_paths), int(n_months), float(rho),
        out.ctypes.data, int(device),
    )
    N.check(rc, "mcr_draw_shocks_host_rng")
    return out


def eval_helper_host(which: int, params: Optional[McrParams], rows, device: int = 0) -> np.ndarray:
    """Evaluate one of the scalar device functions (MCR_HELPER_*) on the GPU for each input row."""
    N.require_device()
    n_in, n_out = N.helper_arity(which)
    a = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, n_in))
    out = np.empty((a.shape[0], n_out), dtype=np.float64)
    rc = N.load_library().mcr_eval_helper_host(
        int(which), C.byref(params) if params is not None else None, a.ctypes.data,
        out.ctypes.data, a.shape[0], int(device),
    )
    N.check(rc, "mcr_eval_helper_host")
    return out


# ---------------------------------------------------------------------------------------------
# Yearly bins: the fan chart without a trajectory slab (mcr_run_year_bins_rng)
# ---------------------------------------------------------------------------------------------
def glide_table(glide_path):
    """The table of a glide path as the ABI takes it, a ``c_double`` array: `glide_path` is a non-empty sequence of
    ``allocation_inv1_pct`` values, one per whole year from today, or an object with such a ``weights`` attribute
    (`allocation.GlidePath`).  The library checks the values."""
    weights = tuple(float(w) for w in getattr(glide_path, "weights", glide_path))
    if not weights:
        raise ValueError("a glide path has at least one weight")
    return (C.c_double * len(weights))(*weights)


def year_edge_array(edges, what: str = "edges") -> np.ndarray:
    """Bin edges of a yearly-bins table as the contiguous float64 array the ABI wants; ``ValueError`` unless they are
    finite, ascending (equal neighbours allowed: zero-width bins) and 2..MCR_MAX_YEAR_BINS+1 long."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
    if not (2 <= e.shape[0] <= N.MCR_MAX_YEAR_BINS + 1):
        raise ValueError(f"{what}: need 2..{N.MCR_MAX_YEAR_BINS + 1} edges, got {e.shape[0]}")
    if not np.all(np.isfinite(e)) or np.any(e[1:] < e[:-1]):
        raise ValueError(f"{what} must be finite and increase monotonically")
    return e


def default_year_edges(n_bins: int = 256, lo: float = 1.0, hi: float = 1e12) -> np.ndarray:
    """Edges for balances in dollars: bin 0 = ``[0, lo)`` holds the exact zeros of failed paths (and the dust below one
    dollar) on its own, the other ``n_bins - 1`` bins are log-spaced from ``lo`` to ``hi`` — a constant RELATIVE width of
    ``(hi / lo) ** (1 / (n_bins - 1))``: 11.4 % at 256 bins, 55 % at 64."""
    n_bins = int(n_bins)
    if not (2 <= n_bins <= N.MCR_MAX_YEAR_BINS):
        raise ValueError(f"default_year_edges: n_bins must be 2..{N.MCR_MAX_YEAR_BINS}, got {n_bins}")
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError("default_year_edges: need 0 < lo < hi, both finite")
    return np.concatenate(([0.0], np.geomspace(float(lo), float(hi), n_bins)))


def default_wr_edges(n_bins: int = 256, hi: float = 100.0) -> np.ndarray:
    """Edges for yearly withdrawal rates in percent of the start balance: ``n_bins`` equal bins over ``[0, hi]``
    (0.39 points wide at 256 bins); rates above ``hi`` land in the `above` cell."""
    n_bins = int(n_bins)
    if not (1 <= n_bins <= N.MCR_MAX_YEAR_BINS):
        raise ValueError(f"default_wr_edges: n_bins must be 1..{N.MCR_MAX_YEAR_BINS}, got {n_bins}")
    if not (np.isfinite(hi) and hi > 0.0):
        raise ValueError("default_wr_edges: need a finite hi > 0")
    return np.linspace(0.0, float(hi), n_bins + 1)


#: (name, rows, cells) of the blocks of a yearly-bins result, in the order of the one vector; T / ry / nb / nw filled in
def _year_bins_layout(sz: McrSizes, n_bins: int, n_wr_bins: int, n_m_bins: Optional[int] = None):
    """``n_m_bins`` (a launch under a spending rule): the rule's two blocks BEHIND the others, so the plain layout is a prefix."""
    T, ry = sz.trajectory_len, sz.retirement_years
    plain = (
        ("counters", 1, N.MCR_N_COUNTERS), ("wr_obs_counts", 1, ry), ("ruin_year_bins", 1, sz.ruin_bins),
        ("trajectory_bins", T, n_bins + 2), ("real_trajectory_bins", T, n_bins + 2), ("wr_bins", ry, n_wr_bins + 2),
        ("final_success_bins", 1, n_bins + 2),
    )
    if n_m_bins is None:
        return plain
    return plain + (("rule_year_counts", ry, N.MCR_RULE_N_COUNTS), ("multiplier_bins", ry, int(n_m_bins) + 2))


_YEAR_BINS_TABLES = ("trajectory_bins", "real_trajectory_bins", "wr_bins", "rule_year_counts", "multiplier_bins")


def split_year_bins(vec, sz: McrSizes, n_bins: int, n_wr_bins: int, n_m_bins: Optional[int] = None) -> dict:
    """Named views of the one vector ``[counters | wr_obs | ruin | trajectory | real | wr | final_success]`` (numpy
    array or torch tensor): tables ``[rows, cells]``, the others flat.  With ``n_m_bins`` (a launch under a spending rule)
    the vector ends ``... | rule_year_counts[ry][4] | multiplier_bins[ry][n_m_bins + 2]]``."""
    out, at = {}, 0
    for name, rows, cells in _year_bins_layout(sz, n_bins, n_wr_bins, n_m_bins):
        v = vec[at:at + rows * cells]
        out[name] = v.reshape(rows, cells) if name in _YEAR_BINS_TABLES else v
        at += rows * cells
    assert at == vec.shape[0]
    return out


class YearBinsBatch:
    """The integer block of a yearly-bins run resident in HBM: ONE contiguous int64 device vector ``reduce_vec`` =
    ``[counters | wr_obs_counts | ruin_year_bins | trajectory_bins | real_trajectory_bins | wr_bins | final_success_bins]``
    with named views into it, accumulated into by every :meth:`launch` (``mcr_run_year_bins_rng`` on torch's current
    stream).  Nothing is kept per path: the vector is all a multi-GPU caller has to sum.

    ``rule`` (a `spending_rules.SpendingRule` or ``McrSpendingRule``): the paths spend under that guardrail
    (``mcr_run_rule_year_bins_rng``), and the vector gains two blocks behind the others,
    ``[... | final_success_bins | rule_year_counts[ry][4] | multiplier_bins[ry][nm + 2]]``, the multipliers binned on
    ``m_edges`` (default: `default_multiplier_edges`).

    ``glide_path`` (a sequence of ``allocation_inv1_pct`` values, one per whole year from today, or anything with a
    ``weights`` attribute): the paths hold that glide path (``mcr_run_glide_year_bins_rng``); the vector is the plain one.
    A ``rule`` together with a ``glide_path`` is refused with a ``ValueError``."""

    def __init__(self, params: McrParams, working_months: int, edges=None, wr_edges=None, device: int = 0, rule=None, m_edges=None,
                 glide_path=None):
        import torch

        if rule is not None and glide_path is not None:
            raise ValueError("a spending rule together with a glide path is not supported")
        self.glide = None if glide_path is None else glide_table(glide_path)
        N.require_device()
        self.torch = torch
        self.params = params
        self.working_months = int(working_months)
        self.device = int(device)
        self.sizes = query_sizes(params, working_months)
        self.edges = year_edge_array(default_year_edges() if edges is None else edges)
        self.wr_edges = year_edge_array(default_wr_edges() if wr_edges is None else wr_edges, "wr_edges")
        self.n_bins, self.n_wr_bins = self.edges.shape[0] - 1, self.wr_edges.shape[0] - 1
        if rule is None and m_edges is not None:
            raise ValueError("m_edges without a spending rule")
        self.rule = None if rule is None else _rule_record(rule)
        self.m_edges = None if rule is None else year_edge_array(default_multiplier_edges(self.rule) if m_edges is None else m_edges, "m_edges")
        self.n_m_bins = None if rule is None else self.m_edges.shape[0] - 1
        dev = torch.device("cuda", self.device)
        n_words = sum(rows * cells for _, rows, cells in _year_bins_layout(self.sizes, self.n_bins, self.n_wr_bins, self.n_m_bins))
        self.reduce_vec = torch.zeros(n_words, dtype=torch.int64, device=dev)
        for name, view in split_year_bins(self.reduce_vec, self.sizes, self.n_bins, self.n_wr_bins, self.n_m_bins).items():
            setattr(self, name, view)
        self._edges_dev = torch.as_tensor(self.edges, device=dev)
        self._wr_edges_dev = torch.as_tensor(self.wr_edges, device=dev)
        o = McrOutputs()
        o.counters = self.counters.data_ptr()
        o.wr_obs_counts = self.wr_obs_counts.data_ptr()
        o.ruin_year_bins = self.ruin_year_bins.data_ptr()
        y = McrYearBins()
        y.edges, y.n_bins = self._edges_dev.data_ptr(), self.n_bins
        y.wr_edges, y.n_wr_bins = self._wr_edges_dev.data_ptr(), self.n_wr_bins
        y.trajectory_bins = self.trajectory_bins.data_ptr()
        y.real_trajectory_bins = self.real_trajectory_bins.data_ptr()
        y.wr_bins = self.wr_bins.data_ptr()
        y.final_success_bins = self.final_success_bins.data_ptr()
        self._out, self._yb = o, y
        self._rule_yb = None
        if self.rule is not None:
            self._m_edges_dev = torch.as_tensor(self.m_edges, device=dev)
            r = McrRuleYearBins()
            r.m_edges, r.n_m_bins = self._m_edges_dev.data_ptr(), self.n_m_bins
            r.multiplier_bins = self.multiplier_bins.data_ptr()
            r.year_counts = self.rule_year_counts.data_ptr()
            self._rule_yb = r
        self._lib = N.load_library()

    def zero(self) -> None:
        self.reduce_vec.zero_()

    def launch(self, seed, stream_id: int, path_begin: int, n_paths: int) -> None:
        """Enqueue one launch over global paths ``[path_begin, path_begin + n_paths)`` on the current stream; the tables
        accumulate.  ``seed``: int (Philox key) or an ``McrRng`` descriptor."""
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        rng = _as_rng(seed, self.device)
        if self.rule is not None:
            rc = self._lib.mcr_run_rule_year_bins_rng(
                C.byref(self.params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), self.working_months,
                C.byref(self.rule), C.byref(self._out), C.byref(self._yb), C.byref(self._rule_yb), self.device, C.c_void_p(stream),
            )
            N.check(rc, "mcr_run_rule_year_bins_rng")
            return
        if self.glide is not None:
            rc = self._lib.mcr_run_glide_year_bins_rng(
                C.byref(self.params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), self.working_months,
                self.glide, len(self.glide), C.byref(self._out), C.byref(self._yb), self.device, C.c_void_p(stream),
            )
            N.check(rc, "mcr_run_glide_year_bins_rng")
            return
        rc = self._lib.mcr_run_year_bins_rng(
            C.byref(self.params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), self.working_months,
            C.byref(self._out), C.byref(self._yb), self.device, C.c_void_p(stream),
        )
        N.check(rc, "mcr_run_year_bins_rng")

    def host(self) -> Dict[str, np.ndarray]:
        """The block on the host (synchronises): named numpy arrays, plus the edges."""
        res = split_year_bins(self.reduce_vec.cpu().numpy(), self.sizes, self.n_bins, self.n_wr_bins, self.n_m_bins)
        res["edges"], res["wr_edges"] = self.edges, self.wr_edges
        if self.rule is not None:
            res["m_edges"] = self.m_edges
        return res


def run_year_bins_host(
    params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
    edges=None, wr_edges=None, device: int = 0, devices: Optional[Sequence[int]] = None,
    path_seeds: Optional[np.ndarray] = None, into: Optional[Dict[str, np.ndarray]] = None,
) -> Dict[str, np.ndarray]:
    """Yearly bins of paths ``[path_begin, path_begin + n_paths)`` through host buffers (``mcr_run_year_bins_host_rng``;
    ``devices``: ``mcr_run_year_bins_multi_host_rng``).  Returns uint64 arrays ``counters`` ``[2]``, ``wr_obs_counts``
    ``[ry]``, ``ruin_year_bins`` ``[ry+2]``, ``trajectory_bins`` / ``real_trajectory_bins`` ``[T, n_bins+2]``, ``wr_bins``
    ``[ry, n_wr_bins+2]``, ``final_success_bins`` ``[n_bins+2]`` and the two edge arrays.  ``into``: a previous result to
    accumulate into (same edges).  There are no injected shocks on this route: the entry points take none."""
    lib = N.load_library()
    N.require_device()
    sz = query_sizes(params, working_months)
    e = year_edge_array(default_year_edges() if edges is None else edges)
    we = year_edge_array(default_wr_edges() if wr_edges is None else wr_edges, "wr_edges")
    nb, nw = e.shape[0] - 1, we.shape[0] - 1
    if into is not None:
        res = into
        if not (np.array_equal(res["edges"], e) and np.array_equal(res["wr_edges"], we)):
            raise ValueError("`into` was binned on other edges")
    else:
        res = {name: np.zeros((rows, cells) if rows > 1 or name in ("trajectory_bins", "real_trajectory_bins", "wr_bins") else cells,
                              dtype=np.uint64)
               for name, rows, cells in _year_bins_layout(sz, nb, nw)}
        res["edges"], res["wr_edges"] = e, we
    o = McrOutputs()
    o.counters = res["counters"].ctypes.data
    o.wr_obs_counts = res["wr_obs_counts"].ctypes.data
    o.ruin_year_bins = res["ruin_year_bins"].ctypes.data
    y = McrYearBins()
    y.edges, y.n_bins, y.wr_edges, y.n_wr_bins = e.ctypes.data, nb, we.ctypes.data, nw
    for name in ("trajectory_bins", "real_trajectory_bins", "wr_bins", "final_success_bins"):
        setattr(y, name, res[name].ctypes.data)
    rng = _as_rng(seed)
    seeds_arr = None
    if path_seeds is not None:
        seeds_arr = np.ascontiguousarray(path_seeds, dtype=np.uint32)
        if seeds_arr.shape != (int(n_paths),):
            raise ValueError("path_seeds must have one uint32 per path")
        rng.path_seeds = seeds_arr.ctypes.data
    if devices is not None:
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        rc = lib.mcr_run_year_bins_multi_host_rng(
            C.byref(params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), int(working_months),
            C.byref(o), C.byref(y), devs, len(devices))
        N.check(rc, "mcr_run_year_bins_multi_host_rng")
        return res
    rc = lib.mcr_run_year_bins_host_rng(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), int(working_months),
        C.byref(o), C.byref(y), int(device))
    N.check(rc, "mcr_run_year_bins_host_rng")
    return res


# ---------------------------------------------------------------------------------------------
# Device-resident batches (torch = device memory + stream plumbing only)
# ---------------------------------------------------------------------------------------------
class DeviceBatch:
    """Outputs of one (possibly multi-launch) batch kept resident in HBM.

    ``want``: ``"count"`` (counters/bins only), ``"summary"`` (+ per-path fields) or
    ``"full"`` (+ time-major trajectories).  Tensors are allocated once and reused; launches
    go to torch's current stream through ``mcr_run_batch`` (device pointers).
    """

    def __init__(self, params: McrParams, working_months: int, n_paths: int, want: str = "count",
                 device: int = 0, hist_edges=None):
        import torch

        if want not in ("count", "summary", "full"):
            raise ValueError(want)
        N.require_device()
        self.torch = torch
        self.params = params
        self.working_months = int(working_months)
        self.n_paths = int(n_paths)
        self.want = want
        self.device = int(device)
        self.sizes = query_sizes(params, working_months)
        dev = torch.device("cuda", self.device)
        self.stride = (self.n_paths + 63) // 64 * 64
        f64, i64 = torch.float64, torch.int64
        # counters | wr_obs_counts | ruin_year_bins live in ONE int64 vector: the path's single exchange step
        # across GPUs is one all-reduce(sum) of it
        ry_ = self.sizes.retirement_years
        self.hist_edges = None if hist_edges is None else hist_edge_array(hist_edges)
        n_hist = 0 if self.hist_edges is None else self.hist_edges.shape[0] - 1
        n_fixed = N.MCR_N_COUNTERS + ry_ + self.sizes.ruin_bins
        self.reduce_vec = torch.zeros(n_fixed + n_hist, dtype=i64, device=dev)
        self.counters = self.reduce_vec[:N.MCR_N_COUNTERS]
        self.wr_obs_counts = self.reduce_vec[N.MCR_N_COUNTERS:N.MCR_N_COUNTERS + ry_]
        self.ruin_year_bins = self.reduce_vec[N.MCR_N_COUNTERS + ry_:n_fixed]
        self.hist_bins = self.reduce_vec[n_fixed:] if n_hist else None
        self._hist_edges_dev = torch.as_tensor(self.hist_edges, device=dev) if n_hist else None
        self.summary = {}
        self.success = None
        self.trajectory = self.real_trajectory = self.withdrawal_rate_trajectory = None
        if want in ("summary", "full"):
            for k in SUMMARY_FIELDS:
                self.summary[k] = torch.empty(self.n_paths, dtype=f64, device=dev)
            self.success = torch.empty(self.n_paths, dtype=torch.uint8, device=dev)
        self.slab = None
        if want == "full":
            # one [2T+ry, stride] slab (nominal | real | withdrawal-rate rows) so the quantile bands of all
            # rows come from a single radix-select call
            T, ry = self.sizes.trajectory_len, self.sizes.retirement_years
            self.slab = torch.empty((2 * T + ry, self.stride), dtype=f64, device=dev)
            self.trajectory = self.slab[:T]
            self.real_trajectory = self.slab[T:2 * T]
            self.withdrawal_rate_trajectory = self.slab[2 * T:]
        o = McrOutputs()
        o.path_stride = self.stride
        o.counters = self.counters.data_ptr()
        o.wr_obs_counts = self.wr_obs_counts.data_ptr()
        o.ruin_year_bins = self.ruin_year_bins.data_ptr()
        if n_hist:
            o.hist_edges = self._hist_edges_dev.data_ptr()
            o.hist_bins = self.hist_bins.data_ptr()
            o.hist_n_bins = n_hist
        for k, t in self.summary.items():
            setattr(o, k, t.data_ptr())
        if self.success is not None:
            o.success = self.success.data_ptr()
        if self.trajectory is not None:
            o.trajectory = self.trajectory.data_ptr()
            o.real_trajectory = self.real_trajectory.data_ptr()
            o.withdrawal_rate_trajectory = self.withdrawal_rate_trajectory.data_ptr()
        self._out = o
        self._lib = N.load_library()

    def zero_counters(self) -> None:
        self.reduce_vec.zero_()

    def release_scratch(self) -> None:
        """Drop the selection scratch the aggregation calls cached on this batch (`aggregation.band_quantiles` /
        `row_quantiles(..., scratch_owner=batch)`: ~1.5 GB at 136 rows x 1e7 paths, kept next to the slab for the batch's
        lifetime so that repeated selections do not re-allocate).  The next selection allocates it again."""
        self._rq_scratch = None

    def launch(self, seed, stream_id: int, path_begin: int, n_paths: Optional[int] = None) -> None:
        """Enqueue one kernel launch over ``n_paths`` (default: the whole batch) on the current stream.
        ``seed``: int (Philox key) or an ``McrRng`` descriptor."""
        n = self.n_paths if n_paths is None else int(n_paths)
        if n > self.n_paths:
            raise ValueError("launch larger than the batch buffers")
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        rng = _as_rng(seed, self.device)
        rc = self._lib.mcr_run_batch_rng(
            C.byref(self.params), C.byref(rng), int(stream_id), int(path_begin), n,
            self.working_months, None, C.byref(self._out), self.device, C.c_void_p(stream),
        )
        N.check(rc, "mcr_run_batch_rng")


def probe_months(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months,
                 device: int = 0):
    """Success counters of several candidate working-month counts over the same path range: one
    count-only launch per candidate, run concurrently on the library's side streams (fork/join on
    torch's current stream).  Returns a device int64 tensor ``[len(working_months), 2]`` =
    ``{successes, paths}``; asynchronous (reading it synchronises)."""
    import torch

    N.require_device()
    months = (C.c_int32 * len(working_months))(*[int(m) for m in working_months])
    counts = torch.empty((len(working_months), N.MCR_N_COUNTERS), dtype=torch.int64,
                         device=torch.device("cuda", int(device)))
    if len(working_months) == 0:
        return counts
    rng = _as_rng(seed, int(device))
    stream = torch.cuda.current_stream(int(device)).cuda_stream
    rc = N.load_library().mcr_probe_months_rng(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), months,
        len(working_months), counts.data_ptr(), int(device), C.c_void_p(stream),
    )
    N.check(rc, "mcr_probe_months_rng")
    return counts


def _probe_levels(symbol: str, params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                  levels, device: int):
    """The body of `probe_expenses` / `probe_contributions`: `symbol` is the library entry that takes the levels."""
    import torch

    N.require_device()
    levels = [float(x) for x in levels]
    arr = (C.c_double * max(1, len(levels)))(*levels)
    counts = torch.empty((len(levels), N.MCR_N_COUNTERS), dtype=torch.int64, device=torch.device("cuda", int(device)))
    if not levels:
        return counts
    rng = _as_rng(seed, int(device))
    stream = torch.cuda.current_stream(int(device)).cuda_stream
    rc = getattr(N.load_library(), symbol)(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), int(working_months), arr,
        len(levels), counts.data_ptr(), int(device), C.c_void_p(stream),
    )
    N.check(rc, symbol)
    return counts


def probe_expenses(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                   monthly_expenses, device: int = 0):
    """Success counters of several ``monthly_expenses`` levels at one working-month count over the same path range
    (``mcr_probe_expenses_rng``): level k counts exactly what a count-only launch with ``monthly_expenses =
    monthly_expenses[k]`` counts.  The accumulation runs once and up to ``MCR_MAX_EXPENSE_FANOUT`` levels share each
    path's random numbers.  Returns a device int64 tensor ``[len(monthly_expenses), 2]`` = ``{successes, paths}``;
    asynchronous (reading it synchronises)."""
    return _probe_levels("mcr_probe_expenses_rng", params, seed, stream_id, path_begin, n_paths, working_months,
                         monthly_expenses, device)


def probe_contributions(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                        monthly_contributions, device: int = 0):
    """Success counters of several ``monthly_contribution`` levels at one working-month count over the same path range
    (``mcr_probe_contributions_rng``): level k counts exactly what a count-only launch with ``monthly_contribution =
    monthly_contributions[k]`` counts.  Up to ``MCR_MAX_EXPENSE_FANOUT`` levels share each path's random numbers (the
    levels differ from month 0, so each runs the whole path).  Returns a device int64 tensor
    ``[len(monthly_contributions), 2]`` = ``{successes, paths}``; asynchronous (reading it synchronises)."""
    return _probe_levels("mcr_probe_contributions_rng", params, seed, stream_id, path_begin, n_paths, working_months,
                         monthly_contributions, device)


def _scenario_records(scenarios):
    records = [tuple(float(x) for x in s) for s in scenarios]
    if any(len(r) != 3 for r in records):
        raise ValueError("every scenario is (initial_balance, monthly_contribution, monthly_expenses)")
    return (McrScenario * max(1, len(records)))(*[McrScenario(*r) for r in records]), len(records)


def _income_records(options):
    options = [tuple(o) for o in options]
    if any(len(o) != 6 for o in options):
        raise ValueError("every option is (initial_balance, monthly_contribution, monthly_expenses, monthly_amount_today, "
                         "start_at_age, duration_years)")
    records = [McrIncomeOption(*(float(x) for x in o[:5]), -1 if o[5] is None else int(o[5]), 0) for o in options]
    return (McrIncomeOption * max(1, len(records)))(*records), len(records)


def _assumption_records(records):
    records = [tuple(float(x) for x in r) for r in records]
    if any(len(r) != 10 for r in records):
        raise ValueError("every record holds the ten fields of mcr_assumptions")
    return (McrAssumptions * max(1, len(records)))(*[McrAssumptions(*r) for r in records]), len(records)


def _probe_records(symbol: str, params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                   record_args, n: int, device: int, joint: bool = False, masks=True, outcomes=None, after_counts=()):
    """The body of the record probes: `symbol` is the library entry, `record_args` what it takes between `working_months` and
    the record count.  Plain: returns `counts`.  `joint`: the ``*_joint_rng`` entry; returns ``(counts, joint, extremes,
    masks)`` (`masks` falsy: the library keeps them in scratch of its own and None is returned in their place).  `outcomes`:
    the ``*_outcomes_rng`` entry; ``(final_balance, years_to_ruin, path_stride)`` with each row argument True (allocate),
    falsy (not requested) or a float64 device tensor ``[n, path_stride]`` to write into; returns ``(counts, final_rows,
    ruin_rows)``.  `after_counts`: what the entry takes right behind `counts` (the rule probes' year counts)."""
    import torch

    N.require_device()
    dev = torch.device("cuda", int(device))
    counts = torch.empty((n, N.MCR_N_COUNTERS), dtype=torch.int64, device=dev)
    outs = []
    if outcomes is not None:
        want_final, want_ruin, stride = outcomes
        stride = (int(n_paths) + 63) // 64 * 64 if stride is None else int(stride)

        def row_slab(want):
            if want is None or want is False:
                return None
            if want is True:
                return torch.empty((n, stride), dtype=torch.float64, device=dev)
            if not (torch.is_tensor(want) and want.is_cuda and want.dtype == torch.float64 and want.is_contiguous()
                    and tuple(want.shape) == (n, stride)):
                raise ValueError(f"a row slab must be a contiguous float64 device tensor of shape ({n}, {stride})")
            return want

        fin, ruin = row_slab(want_final), row_slab(want_ruin)
        rows = McrOptionOutcomes(fin.data_ptr() if fin is not None and fin.numel() else None,
                                 ruin.data_ptr() if ruin is not None and ruin.numel() else None, stride)
        outs = [C.byref(rows)]
    if joint:
        if n > N.MCR_MAX_JOINT_OPTIONS:
            raise ValueError(f"a joint probe takes at most MCR_MAX_JOINT_OPTIONS = {N.MCR_MAX_JOINT_OPTIONS} options, got {n}")
        alloc = torch.empty if n else torch.zeros       # (the call zeroes or overwrites all three; no options: no call)
        jm = alloc((n, n), dtype=torch.int64, device=dev)
        ex = alloc((2,), dtype=torch.int64, device=dev)
        mk = alloc((n, joint_mask_words(n_paths)), dtype=torch.int64, device=dev) if masks else None
        outs = [mk.data_ptr() if mk is not None and mk.numel() else None, jm.data_ptr() if n else None, ex.data_ptr()]
    if n:
        rng = _as_rng(seed, int(device))
        stream = torch.cuda.current_stream(int(device)).cuda_stream
        rc = getattr(N.load_library(), symbol)(
            C.byref(params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), int(working_months), *record_args,
            n, counts.data_ptr(), *after_counts, *outs, int(device), C.c_void_p(stream),
        )
        N.check(rc, symbol)
    if outcomes is not None:
        return counts, fin, ruin
    return (counts, jm, ex, mk) if joint else counts


def joint_mask_words(n_paths: int) -> int:
    """Words of one option's success mask over `n_paths` paths (``mcr_joint_mask_words``)."""
    return (int(n_paths) + 63) // 64


def probe_scenarios(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                    scenarios, device: int = 0):
    """Success counters of several what-if scenarios at one working-month count over the same path range
    (``mcr_probe_scenarios_rng``).  ``scenarios`` is a sequence of ``(initial_balance, monthly_contribution,
    monthly_expenses)`` 3-tuples; scenario k counts exactly what a count-only launch with those three fields of `params`
    replaced counts.  Up to ``MCR_MAX_EXPENSE_FANOUT`` scenarios share each path's random numbers.  Returns a device int64
    tensor ``[len(scenarios), 2]`` = ``{successes, paths}``; asynchronous (reading it synchronises)."""
    arr, n = _scenario_records(scenarios)
    return _probe_records("mcr_probe_scenarios_rng", params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n, device)


def probe_income(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                 stream_index: int, options, device: int = 0):
    """Success counters of several versions of one income stream at one working-month count over the same path range
    (``mcr_probe_income_rng``).  ``options`` is a sequence of 6-tuples in the order of ``mcr_income_option``:
    ``(initial_balance, monthly_contribution, monthly_expenses, monthly_amount_today, start_at_age, duration_years)`` with
    ``duration_years`` an int or ``None`` (paid for life); option k counts exactly what a count-only launch counts with the
    three money fields of `params` and those three fields of entry ``stream_index`` of its stream list replaced.  Up to
    ``MCR_MAX_EXPENSE_FANOUT`` options share each path's random numbers.  Returns a device int64 tensor ``[len(options), 2]``
    = ``{successes, paths}``; asynchronous (reading it synchronises)."""
    arr, n = _income_records(options)
    return _probe_records("mcr_probe_income_rng", params, seed, stream_id, path_begin, n_paths, working_months,
                          (int(stream_index), arr), n, device)


def probe_assumptions(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                      records, device: int = 0):
    """Success counters of several market-assumption records at one working-month count over the same path range
    (``mcr_probe_assumptions_rng``).  ``records`` is a sequence of 10-tuples in the order of ``mcr_assumptions``:
    ``(initial_balance, monthly_contribution, monthly_expenses, inv1_mu_log, inv1_sigma_log, inf_mu_log, inf_sigma_log,
    prem_mu_log, prem_sigma_log, equity_inflation_rho)``; record k counts exactly what a count-only launch with those ten
    fields of `params` replaced counts.  Up to ``MCR_MAX_EXPENSE_FANOUT`` records share each path's normals.  Returns a
    device int64 tensor ``[len(records), 2]`` = ``{successes, paths}``; asynchronous (reading it synchronises)."""
    arr, n = _assumption_records(records)
    return _probe_records("mcr_probe_assumptions_rng", params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n, device)


def probe_scenarios_joint(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                          scenarios, device: int = 0, masks=True):
    """`probe_scenarios` plus the joint outcomes of its scenarios over the shared paths (``mcr_probe_scenarios_joint_rng``).
    Returns device int64 tensors ``(counts, joint, extremes, masks)``: `counts` as the plain probe's; ``joint[i, j]`` = paths on
    which scenarios i and j both succeed (the diagonal is ``counts[:, 0]``); ``extremes`` = ``{paths on which all succeed,
    paths on which none does}``; ``masks[k]`` = scenario k's success bits, bit b of word w = path ``path_begin + 64 w + b``
    (int64 words: bit 63 is the sign).  At most ``MCR_MAX_JOINT_OPTIONS`` scenarios.  ``masks=None``: the library keeps the
    masks in scratch of its own and None comes back in their place.  Asynchronous (reading a tensor synchronises)."""
    arr, n = _scenario_records(scenarios)
    return _probe_records("mcr_probe_scenarios_joint_rng", params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n,
                          device, joint=True, masks=masks)


def probe_income_joint(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                       stream_index: int, options, device: int = 0, masks=True):
    """`probe_income` plus the joint outcomes of its options (``mcr_probe_income_joint_rng``); returns ``(counts, joint,
    extremes, masks)`` as `probe_scenarios_joint`."""
    arr, n = _income_records(options)
    return _probe_records("mcr_probe_income_joint_rng", params, seed, stream_id, path_begin, n_paths, working_months,
                          (int(stream_index), arr), n, device, joint=True, masks=masks)


def probe_assumptions_joint(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                            records, device: int = 0, masks=True):
    """`probe_assumptions` plus the joint outcomes of its records (``mcr_probe_assumptions_joint_rng``); returns ``(counts,
    joint, extremes, masks)`` as `probe_scenarios_joint`."""
    arr, n = _assumption_records(records)
    return _probe_records("mcr_probe_assumptions_joint_rng", params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n,
                          device, joint=True, masks=masks)


def probe_scenarios_outcomes(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                             scenarios, device: int = 0, final_balance=True, years_to_ruin=True, path_stride: Optional[int] = None):
    """`probe_scenarios` plus the per-path outcomes of its scenarios (``mcr_probe_scenarios_outcomes_rng``).  Returns device
    tensors ``(counts, final_rows, ruin_rows)``: `counts` as the plain probe's; the rows are float64 ``[n, path_stride]``
    (default stride: `n_paths` rounded up to 64; columns at or beyond `n_paths` are never written): ``final_rows[k]`` = the final
    balance of the paths that succeed under scenario k, NaN elsewhere; ``ruin_rows[k]`` = YearsToRuin, NaN on success -- bit
    for bit the columns of a summary batch with scenario k's fields.  ``final_balance`` / ``years_to_ruin``: True, falsy (not
    requested: None comes back) or a tensor to write into.  Asynchronous (reading a tensor synchronises)."""
    arr, n = _scenario_records(scenarios)
    return _probe_records("mcr_probe_scenarios_outcomes_rng", params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n,
                          device, outcomes=(final_balance, years_to_ruin, path_stride))


def probe_income_outcomes(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                          stream_index: int, options, device: int = 0, final_balance=True, years_to_ruin=True,
                          path_stride: Optional[int] = None):
    """`probe_income` plus the per-path outcomes of its options (``mcr_probe_income_outcomes_rng``); returns ``(counts,
    final_rows, ruin_rows)`` as `probe_scenarios_outcomes`."""
    arr, n = _income_records(options)
    return _probe_records("mcr_probe_income_outcomes_rng", params, seed, stream_id, path_begin, n_paths, working_months,
                          (int(stream_index), arr), n, device, outcomes=(final_balance, years_to_ruin, path_stride))


def probe_assumptions_outcomes(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                               records, device: int = 0, final_balance=True, years_to_ruin=True, path_stride: Optional[int] = None):
    """`probe_assumptions` plus the per-path outcomes of its records (``mcr_probe_assumptions_outcomes_rng``); returns
    ``(counts, final_rows, ruin_rows)`` as `probe_scenarios_outcomes`."""
    arr, n = _assumption_records(records)
    return _probe_records("mcr_probe_assumptions_outcomes_rng", params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n,
                          device, outcomes=(final_balance, years_to_ruin, path_stride))


def _allocation_option_records(options):
    records = [tuple(float(x) for x in o) for o in options]
    if any(len(r) != 4 for r in records):
        raise ValueError("every option is (initial_balance, monthly_contribution, monthly_expenses, allocation_inv1_pct)")
    return (N.McrAllocationOption * max(1, len(records)))(*[N.McrAllocationOption(*r) for r in records]), len(records)


def probe_allocations(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                      options, device: int = 0):
    """Success counters of several splits between the two assets (and versions of the three scenario fields) at one
    working-month count over the same path range (``mcr_probe_allocations_rng``).  ``options`` is a sequence of
    ``(initial_balance, monthly_contribution, monthly_expenses, allocation_inv1_pct)`` 4-tuples; option k counts exactly what
    a count-only launch with those four fields of `params` replaced counts.  Up to ``MCR_MAX_EXPENSE_FANOUT`` options share
    each path's random numbers.  Returns a device int64 tensor ``[len(options), 2]`` = ``{successes, paths}``; asynchronous
    (reading it synchronises)."""
    arr, n = _allocation_option_records(options)
    return _probe_records("mcr_probe_allocations_rng", params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n, device)


def probe_allocations_joint(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                            options, device: int = 0, masks=True):
    """`probe_allocations` plus the joint outcomes of its options (``mcr_probe_allocations_joint_rng``); returns ``(counts,
    joint, extremes, masks)`` as `probe_scenarios_joint`."""
    arr, n = _allocation_option_records(options)
    return _probe_records("mcr_probe_allocations_joint_rng", params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n,
                          device, joint=True, masks=masks)


def probe_allocations_outcomes(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                               options, device: int = 0, final_balance=True, years_to_ruin=True, path_stride: Optional[int] = None):
    """`probe_allocations` plus the per-path outcomes of its options (``mcr_probe_allocations_outcomes_rng``); returns
    ``(counts, final_rows, ruin_rows)`` as `probe_scenarios_outcomes`."""
    arr, n = _allocation_option_records(options)
    return _probe_records("mcr_probe_allocations_outcomes_rng", params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n,
                          device, outcomes=(final_balance, years_to_ruin, path_stride))


def _glide_option_records(options):
    """`options`: ``(initial_balance, monthly_contribution, monthly_expenses, weights)`` 4-tuples, `weights` the option's glide
    path (a non-empty sequence of ``allocation_inv1_pct`` values, one per whole year from today).  Returns what the glide
    probes take between ``working_months`` and ``n_options``: the flat table (equal tables are stored once), its length and the
    records."""
    flat, first_of, records = [], {}, []
    for o in options:
        if len(o) != 4:
            raise ValueError("every option is (initial_balance, monthly_contribution, monthly_expenses, weights)")
        weights = tuple(float(w) for w in o[3])
        if not weights:
            raise ValueError("a glide path has at least one weight")
        if weights not in first_of:
            first_of[weights] = len(flat)
            flat.extend(weights)
        records.append(N.McrGlideOption(float(o[0]), float(o[1]), float(o[2]), first_of[weights], len(weights)))
    table = (C.c_double * max(1, len(flat)))(*flat)
    return (table, len(flat), (N.McrGlideOption * max(1, len(records)))(*records)), len(records)


def probe_glide_paths(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                      options, device: int = 0):
    """Success counters of several glide paths (and versions of the three scenario fields) at one working-month count over the
    same path range (``mcr_probe_glide_paths_rng``; include/mcr.h: GLIDE PATH).  ``options`` is a sequence of
    ``(initial_balance, monthly_contribution, monthly_expenses, weights)`` 4-tuples; a constant table counts exactly what
    `probe_allocations` counts for that split.  Up to ``MCR_MAX_EXPENSE_FANOUT`` options share each path's random numbers, and
    a single option runs in the same kernel.  Shapes the glide fan-out does not cover (the NumPy and history streams, the
    generic variant, the exact month) raise the library's ``MCR_ERR_UNSUPPORTED`` error unchanged.  Returns a device int64
    tensor ``[len(options), 2]`` = ``{successes, paths}``; asynchronous (reading it synchronises)."""
    args, n = _glide_option_records(options)
    return _probe_records("mcr_probe_glide_paths_rng", params, seed, stream_id, path_begin, n_paths, working_months, args, n, device)


def probe_glide_paths_joint(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                            options, device: int = 0, masks=True):
    """`probe_glide_paths` plus the joint outcomes of its options (``mcr_probe_glide_paths_joint_rng``); returns ``(counts,
    joint, extremes, masks)`` as `probe_scenarios_joint`."""
    args, n = _glide_option_records(options)
    return _probe_records("mcr_probe_glide_paths_joint_rng", params, seed, stream_id, path_begin, n_paths, working_months, args, n,
                          device, joint=True, masks=masks)


def probe_glide_paths_outcomes(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                               options, device: int = 0, final_balance=True, years_to_ruin=True, path_stride: Optional[int] = None):
    """`probe_glide_paths` plus the per-path outcomes of its options (``mcr_probe_glide_paths_outcomes_rng``); returns
    ``(counts, final_rows, ruin_rows)`` as `probe_scenarios_outcomes`."""
    args, n = _glide_option_records(options)
    return _probe_records("mcr_probe_glide_paths_outcomes_rng", params, seed, stream_id, path_begin, n_paths, working_months, args, n,
                          device, outcomes=(final_balance, years_to_ruin, path_stride))


def _rule_option_records(options):
    """`options`: ``(initial_balance, monthly_contribution, monthly_expenses, rule)`` 4-tuples, `rule` a
    `spending_rules.SpendingRule`, a ready ``McrSpendingRule`` or None (the neutral rule: fixed spending)."""
    records = []
    for o in options:
        o = tuple(o)
        if len(o) != 4:
            raise ValueError("every option is (initial_balance, monthly_contribution, monthly_expenses, rule)")
        rule = N.McrSpendingRule(1.0, 1.0, 0.0, 0.0, 1.0, 1.0) if o[3] is None else _rule_record(o[3])
        records.append(N.McrRuleOption(float(o[0]), float(o[1]), float(o[2]), rule))
    return (N.McrRuleOption * max(1, len(records)))(*records), len(records)


def _probe_rules(symbol: str, params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int,
                 options, device: int, year_counts: bool, **kw):
    import torch

    arr, n = _rule_option_records(options)
    yc = None
    if year_counts:
        N.require_device()
        ry = int(query_sizes(params, working_months).retirement_years)
        alloc = torch.empty if n else torch.zeros       # (the call zeroes it; no options: no call)
        yc = alloc((n, ry, N.MCR_RULE_N_COUNTS), dtype=torch.int64, device=torch.device("cuda", int(device)))
    res = _probe_records(symbol, params, seed, stream_id, path_begin, n_paths, working_months, (arr,), n, device,
                         after_counts=(yc.data_ptr() if yc is not None and yc.numel() else None,), **kw)
    return (res, yc) if torch.is_tensor(res) else (res[0], yc) + tuple(res[1:])


def probe_rules(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int, options,
                device: int = 0, year_counts: bool = True):
    """Success counters and year counts of several spending rules (and versions of the three scenario fields) at one
    working-month count over the same path range (``mcr_probe_rules_rng``).  ``options`` is a sequence of ``(initial_balance,
    monthly_contribution, monthly_expenses, rule)`` 4-tuples, `rule` a `spending_rules.SpendingRule` or None (fixed spending);
    option k counts exactly what a count-only `run_rule` with those three fields of `params` replaced counts under its rule.
    Up to ``MCR_MAX_EXPENSE_FANOUT`` options share each path's random numbers.  Returns device int64 tensors ``(counts,
    year_counts)``: ``[len(options), 2]`` = ``{successes, paths}`` and ``[len(options), ry, MCR_RULE_N_COUNTS]`` (None with
    ``year_counts=False``); asynchronous (reading a tensor synchronises)."""
    return _probe_rules("mcr_probe_rules_rng", params, seed, stream_id, path_begin, n_paths, working_months, options, device, year_counts)


def probe_rules_joint(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int, options,
                      device: int = 0, masks=True, year_counts: bool = True):
    """`probe_rules` plus the joint outcomes of its options (``mcr_probe_rules_joint_rng``); returns ``(counts, year_counts,
    joint, extremes, masks)``, the last three as `probe_scenarios_joint`."""
    return _probe_rules("mcr_probe_rules_joint_rng", params, seed, stream_id, path_begin, n_paths, working_months, options, device,
                        year_counts, joint=True, masks=masks)


def probe_rules_outcomes(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int, options,
                         device: int = 0, final_balance=True, years_to_ruin=True, path_stride: Optional[int] = None,
                         year_counts: bool = True):
    """`probe_rules` plus the per-path outcomes of its options (``mcr_probe_rules_outcomes_rng``); returns ``(counts,
    year_counts, final_rows, ruin_rows)``, the last two as `probe_scenarios_outcomes`."""
    return _probe_rules("mcr_probe_rules_outcomes_rng", params, seed, stream_id, path_begin, n_paths, working_months, options, device,
                        year_counts, outcomes=(final_balance, years_to_ruin, path_stride))


def ruin_month_counts(ruin_rows, n_paths: int, retirement_years: int, into=None, device: Optional[int] = None):
    """Ruin-month counts of YearsToRuin rows (``mcr_ruin_month_counts``): `ruin_rows` is a float64 device tensor ``[n, stride]``
    with ``stride >= n_paths`` (the ``ruin_rows`` of an outcomes probe).  Returns a device int64 tensor ``[n, 12 *
    retirement_years + 1]``: cell ``[k, m]`` = the paths of row k ruined in month m (``rint(12 * years_to_ruin) == m``; NaN =
    never).  `into`: a table of that shape to accumulate into (several path ranges, one table).  Asynchronous."""
    import torch

    N.require_device()
    if not (torch.is_tensor(ruin_rows) and ruin_rows.is_cuda and ruin_rows.dtype == torch.float64 and ruin_rows.dim() == 2):
        raise ValueError("ruin_rows must be a 2-d float64 device tensor")
    if ruin_rows.stride(1) != 1 and ruin_rows.numel():
        raise ValueError("the columns of ruin_rows must be contiguous")
    n, cells = int(ruin_rows.shape[0]), 12 * int(retirement_years) + 1
    if int(retirement_years) < 1:
        raise ValueError("retirement_years must be >= 1")
    if int(ruin_rows.shape[1]) < int(n_paths):
        raise ValueError(f"ruin_rows has {int(ruin_rows.shape[1])} columns for {int(n_paths)} paths")
    device = ruin_rows.device.index if device is None else int(device)
    if into is None:
        into = torch.zeros((n, cells), dtype=torch.int64, device=ruin_rows.device)
    elif not (into.is_cuda and into.dtype == torch.int64 and into.is_contiguous() and tuple(into.shape) == (n, cells)):
        raise ValueError(f"`into` must be a contiguous int64 device tensor of shape ({n}, {cells})")
    if n and int(n_paths):
        stream = torch.cuda.current_stream(device).cuda_stream
        row_stride = int(ruin_rows.stride(0)) if n > 1 else max(int(ruin_rows.shape[1]), int(n_paths))
        rc = N.load_library().mcr_ruin_month_counts(ruin_rows.data_ptr(), row_stride, n, int(n_paths), int(retirement_years),
                                                    into.data_ptr(), device, C.c_void_p(stream))
        N.check(rc, "mcr_ruin_month_counts")
    return into


def joint_counts(masks, n_paths: int, device: Optional[int] = None):
    """The co-occurrence reduction alone (``mcr_joint_counts``): `masks` is a device int64 tensor ``[n, joint_mask_words(n_paths)]``
    of success-mask rows, e.g. rows kept from several joint probes over the same path range.  Returns device int64 tensors
    ``(joint [n, n], extremes [2])``.  Bits beyond `n_paths` in the last word are ignored.  Asynchronous."""
    import torch

    N.require_device()
    if masks.dtype != torch.int64 or masks.dim() != 2 or not masks.is_cuda:
        raise ValueError("masks must be a 2-d int64 device tensor")
    n, words = int(masks.shape[0]), joint_mask_words(n_paths)
    if int(masks.shape[1]) != words:
        raise ValueError(f"masks has {int(masks.shape[1])} words per row; {int(n_paths)} paths take {words}")
    if n > N.MCR_MAX_JOINT_OPTIONS:
        raise ValueError(f"joint counts take at most MCR_MAX_JOINT_OPTIONS = {N.MCR_MAX_JOINT_OPTIONS} rows, got {n}")
    device = masks.device.index if device is None else int(device)
    masks = masks.contiguous()
    alloc = torch.empty if n else torch.zeros           # (the call zeroes both)
    jm = alloc((n, n), dtype=torch.int64, device=masks.device)
    ex = alloc((2,), dtype=torch.int64, device=masks.device)
    if n:
        stream = torch.cuda.current_stream(device).cuda_stream
        rc = N.load_library().mcr_joint_counts(masks.data_ptr() if words else None, n, int(n_paths), jm.data_ptr(), ex.data_ptr(),
                                               device, C.c_void_p(stream))
        N.check(rc, "mcr_joint_counts")
    return jm, ex


def probe_grid(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months, levels_2d,
               device: int = 0):
    """Success counters of a grid of working-month counts x ``monthly_expenses`` levels over the same path range
    (``mcr_probe_grid_rng``): cell ``[c, k]`` counts exactly what a count-only launch at ``working_months[c]`` with
    ``monthly_expenses = levels_2d[c][k]`` counts.  ``levels_2d`` is rectangular, one row per month (rows may differ).  The
    accumulation runs once for every month and one launch per level group covers all of them.  Returns a device int64
    tensor ``[len(working_months), n_levels, 2]`` = ``{successes, paths}``; asynchronous (reading it synchronises)."""
    import torch

    N.require_device()
    months, n_levels, marr, larr = _grid_arrays(working_months, levels_2d)
    counts = torch.empty((len(months), n_levels, N.MCR_N_COUNTERS), dtype=torch.int64,
                         device=torch.device("cuda", int(device)))
    if not months or n_levels == 0:
        return counts
    rng = _as_rng(seed, int(device))
    stream = torch.cuda.current_stream(int(device)).cuda_stream
    rc = N.load_library().mcr_probe_grid_rng(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), marr, len(months), larr, n_levels,
        counts.data_ptr(), int(device), C.c_void_p(stream),
    )
    N.check(rc, "mcr_probe_grid_rng")
    return counts


def _grid_arrays(working_months, levels_2d):
    """The months and the rectangular level rows of a grid probe as the C ABI takes them: ``(months, n_levels, int32 array,
    row-major double array)``."""
    months = [int(m) for m in working_months]
    rows = [[float(x) for x in row] for row in levels_2d]
    if len(rows) != len(months):
        raise ValueError(f"levels_2d has {len(rows)} rows for {len(months)} working months")
    n_levels = len(rows[0]) if rows else 0
    if any(len(r) != n_levels for r in rows):
        raise ValueError("levels_2d must be rectangular")
    flat = [x for r in rows for x in r]
    return months, n_levels, (C.c_int32 * max(1, len(months)))(*months), (C.c_double * max(1, len(flat)))(*flat)


def probe_rule_grid(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months, levels_2d, rule,
                    device: int = 0, year_counts: bool = True):
    """`probe_grid` under ONE spending rule (``mcr_probe_rule_grid_rng``): cell ``[c, k]`` counts exactly what a count-only
    `run_rule` at ``working_months[c]`` with ``monthly_expenses = levels_2d[c][k]`` counts under `rule` (a
    `spending_rules.SpendingRule` or ``McrSpendingRule``), year counts included.  A rule acts only after retirement, so the
    accumulation runs once for every month and one launch per level group covers all rows.  Returns device int64 tensors
    ``(counts [R, L, 2], year_counts [R, L, ry, MCR_RULE_N_COUNTS])`` (the second None with ``year_counts=False``);
    asynchronous (reading a tensor synchronises)."""
    import torch

    N.require_device()
    months, n_levels, marr, larr = _grid_arrays(working_months, levels_2d)
    dev = torch.device("cuda", int(device))
    empty = not months or n_levels == 0
    alloc = torch.zeros if empty else torch.empty         # (the call zeroes both; an empty grid: no call)
    counts = alloc((len(months), n_levels, N.MCR_N_COUNTERS), dtype=torch.int64, device=dev)
    yc = None
    if year_counts:
        ry = int(query_sizes(params, months[0] if months else 0).retirement_years)
        yc = alloc((len(months), n_levels, ry, N.MCR_RULE_N_COUNTS), dtype=torch.int64, device=dev)
    if empty:
        return counts, yc
    rng = _as_rng(seed, int(device))
    record = _rule_record(rule)
    stream = torch.cuda.current_stream(int(device)).cuda_stream
    rc = N.load_library().mcr_probe_rule_grid_rng(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), marr, len(months), larr, n_levels,
        C.byref(record), counts.data_ptr(), yc.data_ptr() if yc is not None else None, int(device), C.c_void_p(stream),
    )
    N.check(rc, "mcr_probe_rule_grid_rng")
    return counts, yc


def _rule_record(rule):
    """`rule`: a `spending_rules.SpendingRule` or a ready ``McrSpendingRule``."""
    return rule if isinstance(rule, N.McrSpendingRule) else rule.record()


def run_rule(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int, rule,
             want: str = "count", multipliers: bool = False, device: int = 0, out_extra: Optional[dict] = None):
    """One launch under a spending rule (``mcr_run_rule_rng``) into device tensors, asynchronous on torch's current stream
    (reading a tensor synchronises).  Returns a dict: ``counts`` = one int64 vector ``[2 + 4 ry]``, the counters followed by
    ``year_counts`` row-major (one all-reduce sums it across ranks); with ``want="summary"`` the six float summary fields
    and ``success`` (uint8); with ``multipliers`` the rows ``[ry, n_paths]`` (NaN for a year the path does not begin).
    ``out_extra``: further ``McrOutputs`` fields by name (device addresses), for callers that test what the entry point
    refuses."""
    import torch

    if want not in ("count", "summary"):
        raise ValueError(want)
    N.require_device()
    n = int(n_paths)
    sz = query_sizes(params, working_months)
    ry = int(sz.retirement_years)
    dev = torch.device("cuda", int(device))
    res = {"counts": torch.zeros(N.MCR_N_COUNTERS + N.MCR_RULE_N_COUNTS * ry, dtype=torch.int64, device=dev)}
    o = McrOutputs()
    o.path_stride = n
    o.counters = res["counts"].data_ptr()
    if want == "summary":
        for k in SUMMARY_FIELDS:
            res[k] = torch.empty(n, dtype=torch.float64, device=dev)
            setattr(o, k, res[k].data_ptr())
        res["success"] = torch.empty(n, dtype=torch.uint8, device=dev)
        o.success = res["success"].data_ptr()
    for k, v in (out_extra or {}).items():
        setattr(o, k, v)
    ro = N.McrRuleOutputs()
    ro.year_counts = res["counts"][N.MCR_N_COUNTERS:].data_ptr()
    ro.path_stride = n
    if multipliers:
        res["multipliers"] = torch.empty((ry, n), dtype=torch.float64, device=dev)
        ro.multipliers = res["multipliers"].data_ptr()
    rec = _rule_record(rule)
    rng = _as_rng(seed, int(device))
    stream = torch.cuda.current_stream(int(device)).cuda_stream
    rc = N.load_library().mcr_run_rule_rng(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), n, int(working_months), C.byref(rec), C.byref(o),
        C.byref(ro), int(device), C.c_void_p(stream),
    )
    N.check(rc, "mcr_run_rule_rng")
    return res


def run_rule_host(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int, rule,
                  want: str = "count", multipliers: bool = False, device: int = 0) -> Dict[str, np.ndarray]:
    """`run_rule` with numpy arrays out: ``counters`` ``[2]``, ``year_counts`` ``[ry, 4]`` (columns ``MCR_RULE_ALIVE``,
    ``_CUT``, ``_FLOOR``, ``_RAISED``), with ``want="summary"`` the summary fields and ``success`` as `run_batch_host`
    returns them, with ``multipliers`` the rows ``[ry, n_paths]``."""
    res = run_rule(params, seed, stream_id, path_begin, n_paths, working_months, rule, want=want, multipliers=multipliers,
                   device=device)
    out = {k: v.cpu().numpy() for k, v in res.items() if k != "counts"}
    counts = res["counts"].cpu().numpy()
    out["counters"] = counts[:N.MCR_N_COUNTERS].astype(np.uint64)
    out["year_counts"] = counts[N.MCR_N_COUNTERS:].reshape(-1, N.MCR_RULE_N_COUNTS).astype(np.uint64)
    return out


# ---------------------------------------------------------------------------------------------
# Yearly bins under a spending rule: the fan charts of balance and spending (mcr_run_rule_year_bins_rng)
# ---------------------------------------------------------------------------------------------
def default_multiplier_edges(rule, n_bins: int = 64) -> np.ndarray:
    """Edges for the spending multiplier: ``n_bins`` equal bins over ``[floor, ceiling]``, the range the rule keeps it in.
    The neutral rule's range may be the single point 1.0: zero-width bins, which are legal (every m = 1 lands in the last)."""
    n_bins = int(n_bins)
    if not (1 <= n_bins <= N.MCR_MAX_YEAR_BINS):
        raise ValueError(f"default_multiplier_edges: n_bins must be 1..{N.MCR_MAX_YEAR_BINS}, got {n_bins}")
    rec = _rule_record(rule)
    return np.linspace(float(rec.floor), float(rec.ceiling), n_bins + 1)


def run_rule_year_bins_host(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int, rule,
                            edges=None, wr_edges=None, m_edges=None, device: int = 0,
                            into: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """`run_year_bins_host` under a spending rule (``mcr_run_rule_year_bins_host_rng``, one device): its arrays for paths
    that spend ``(monthly_expenses m) price``, and ``rule_year_counts`` ``[ry, 4]`` (``mcr_run_rule_rng``'s year counts),
    ``multiplier_bins`` ``[ry, n_m_bins+2]`` (row ``y``: the multipliers of the paths that begin year ``y`` alive) and
    ``m_edges``.  ``into``: a previous result to accumulate into (same edges)."""
    lib = N.load_library()
    N.require_device()
    sz = query_sizes(params, working_months)
    rec = _rule_record(rule)
    e = year_edge_array(default_year_edges() if edges is None else edges)
    we = year_edge_array(default_wr_edges() if wr_edges is None else wr_edges, "wr_edges")
    me = year_edge_array(default_multiplier_edges(rec) if m_edges is None else m_edges, "m_edges")
    nb, nw, nm = e.shape[0] - 1, we.shape[0] - 1, me.shape[0] - 1
    if into is not None:
        res = into
        if not (np.array_equal(res["edges"], e) and np.array_equal(res["wr_edges"], we) and np.array_equal(res["m_edges"], me)):
            raise ValueError("`into` was binned on other edges")
    else:
        res = {name: np.zeros((rows, cells) if name in _YEAR_BINS_TABLES else cells, dtype=np.uint64)
               for name, rows, cells in _year_bins_layout(sz, nb, nw, nm)}
        res["edges"], res["wr_edges"], res["m_edges"] = e, we, me
    o = McrOutputs()
    o.counters = res["counters"].ctypes.data
    o.wr_obs_counts = res["wr_obs_counts"].ctypes.data
    o.ruin_year_bins = res["ruin_year_bins"].ctypes.data
    y = McrYearBins()
    y.edges, y.n_bins, y.wr_edges, y.n_wr_bins = e.ctypes.data, nb, we.ctypes.data, nw
    for name in ("trajectory_bins", "real_trajectory_bins", "wr_bins", "final_success_bins"):
        setattr(y, name, res[name].ctypes.data)
    r = McrRuleYearBins()
    r.m_edges, r.n_m_bins = me.ctypes.data, nm
    r.multiplier_bins = res["multiplier_bins"].ctypes.data
    r.year_counts = res["rule_year_counts"].ctypes.data
    rng = _as_rng(seed)
    rc = lib.mcr_run_rule_year_bins_host_rng(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), int(working_months), C.byref(rec),
        C.byref(o), C.byref(y), C.byref(r), int(device))
    N.check(rc, "mcr_run_rule_year_bins_host_rng")
    return res


# ---------------------------------------------------------------------------------------------
# Whole-path launches under a glide path (mcr_run_glide_rng, mcr_run_glide_year_bins_host_rng; include/mcr.h: GLIDE PATH)
# ---------------------------------------------------------------------------------------------
def run_glide(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int, glide_path,
              want: str = "counts", device: int = 0, out_extra: Optional[dict] = None):
    """One launch under a glide path (``mcr_run_glide_rng``) into device tensors, asynchronous on torch's current stream
    (reading a tensor synchronises).  `glide_path`: what `glide_table` takes.  Returns a dict: ``counts`` = one int64 vector
    ``[2 + ry + (ry + 2)]`` = ``[counters | wr_obs_counts | ruin_year_bins]`` (one all-reduce sums it across ranks), which is all
    of ``want="counts"``; with
    ``want="summary"`` the six float summary fields and ``success`` (uint8).  ``out_extra``: further ``McrOutputs`` fields by
    name (device addresses), for callers that test what the entry point refuses."""
    import torch

    if want not in ("counts", "summary"):
        raise ValueError(want)
    table = glide_table(glide_path)
    N.require_device()
    n = int(n_paths)
    sz = query_sizes(params, working_months)
    ry = int(sz.retirement_years)
    dev = torch.device("cuda", int(device))
    res = {"counts": torch.zeros(N.MCR_N_COUNTERS + ry + int(sz.ruin_bins), dtype=torch.int64, device=dev)}
    o = McrOutputs()
    o.path_stride = n
    o.counters = res["counts"].data_ptr()
    o.wr_obs_counts = res["counts"][N.MCR_N_COUNTERS:].data_ptr()
    o.ruin_year_bins = res["counts"][N.MCR_N_COUNTERS + ry:].data_ptr()
    if want == "summary":
        for k in SUMMARY_FIELDS:
            res[k] = torch.empty(n, dtype=torch.float64, device=dev)
            setattr(o, k, res[k].data_ptr())
        res["success"] = torch.empty(n, dtype=torch.uint8, device=dev)
        o.success = res["success"].data_ptr()
    for k, v in (out_extra or {}).items():
        setattr(o, k, v)
    rng = _as_rng(seed, int(device))
    stream = torch.cuda.current_stream(int(device)).cuda_stream
    rc = N.load_library().mcr_run_glide_rng(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), n, int(working_months), table, len(table), C.byref(o),
        int(device), C.c_void_p(stream),
    )
    N.check(rc, "mcr_run_glide_rng")
    return res


def run_glide_host(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int, glide_path,
                   want: str = "counts", device: int = 0) -> Dict[str, np.ndarray]:
    """`run_glide` with numpy arrays out: ``counters`` ``[2]``, ``wr_obs_counts`` ``[ry]``, ``ruin_year_bins`` ``[ry + 2]``, and
    with ``want="summary"`` the summary fields and ``success`` as `run_batch_host` returns them."""
    res = run_glide(params, seed, stream_id, path_begin, n_paths, working_months, glide_path, want=want, device=device)
    out = {k: v.cpu().numpy() for k, v in res.items() if k != "counts"}
    counts = res["counts"].cpu().numpy().astype(np.uint64)
    ry = int(query_sizes(params, working_months).retirement_years)
    out["counters"] = counts[:N.MCR_N_COUNTERS]
    out["wr_obs_counts"] = counts[N.MCR_N_COUNTERS:N.MCR_N_COUNTERS + ry]
    out["ruin_year_bins"] = counts[N.MCR_N_COUNTERS + ry:]
    return out


def run_glide_year_bins_host(params: McrParams, seed, stream_id: int, path_begin: int, n_paths: int, working_months: int, glide_path,
                             edges=None, wr_edges=None, device: int = 0,
                             into: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """`run_year_bins_host` under a glide path (``mcr_run_glide_year_bins_host_rng``, one device): the same arrays for paths
    whose split follows `glide_path` (what `glide_table` takes).  ``into``: a previous result to accumulate into (same edges)."""
    lib = N.load_library()
    table = glide_table(glide_path)
    N.require_device()
    sz = query_sizes(params, working_months)
    e = year_edge_array(default_year_edges() if edges is None else edges)
    we = year_edge_array(default_wr_edges() if wr_edges is None else wr_edges, "wr_edges")
    nb, nw = e.shape[0] - 1, we.shape[0] - 1
    if into is not None:
        res = into
        if not (np.array_equal(res["edges"], e) and np.array_equal(res["wr_edges"], we)):
            raise ValueError("`into` was binned on other edges")
    else:
        res = {name: np.zeros((rows, cells) if name in _YEAR_BINS_TABLES else cells, dtype=np.uint64)
               for name, rows, cells in _year_bins_layout(sz, nb, nw)}
        res["edges"], res["wr_edges"] = e, we
    o = McrOutputs()
    o.counters = res["counters"].ctypes.data
    o.wr_obs_counts = res["wr_obs_counts"].ctypes.data
    o.ruin_year_bins = res["ruin_year_bins"].ctypes.data
    y = McrYearBins()
    y.edges, y.n_bins, y.wr_edges, y.n_wr_bins = e.ctypes.data, nb, we.ctypes.data, nw
    for name in ("trajectory_bins", "real_trajectory_bins", "wr_bins", "final_success_bins"):
        setattr(y, name, res[name].ctypes.data)
    rng = _as_rng(seed)
    rc = lib.mcr_run_glide_year_bins_host_rng(
        C.byref(params), C.byref(rng), int(stream_id), int(path_begin), int(n_paths), int(working_months), table, len(table),
        C.byref(o), C.byref(y), int(device))
    N.check(rc, "mcr_run_glide_year_bins_host_rng")
    return res
