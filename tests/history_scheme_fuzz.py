"""The two other schemes of the history stream (include/mcr.h: MCR_HISTORY_STATIONARY, MCR_HISTORY_COHORTS) restated on the
CPU, and the oracle's answer to a plan on them.

Written from the header's recipes, independently of the library: `stationary_rows` takes every path from row 0 in NumPy
uint64 arithmetic with `history_fuzz.philox4x32_10` (held to the oracle's Philox by tests/test_history_cpu.py), and
`cohort_rows` takes `path mod H` with Python integers.  The oracle takes the gathered rows through `injected_shocks`, as it
does for the block scheme (tests/history_fuzz.py)."""

from __future__ import annotations

import numpy as np

import history_fuzz as HF

BLOCK, STATIONARY, COHORTS = 0, 1, 2
NAMES = {STATIONARY: "stationary", COHORTS: "cohorts"}
_U32 = np.uint64(32)


def stationary_rows(seed: int, stream: int, path_begin: int, n: int, n_rows: int, H: int, B: int, restarts: bool = False):
    """[n, n_rows] int64: the row of the record that shock row r of global path path_begin + i reads (`restarts`: also the
    [n, n_rows] restart flags)."""
    n, n_rows = int(n), int(n_rows)
    path = np.array([(int(path_begin) + i) & 0xFFFFFFFFFFFFFFFF for i in range(n)], dtype=np.uint64)
    lo, hi = path & HF.M32, path >> _U32
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    n_q = (n_rows + 1) // 2                                   # Philox block q serves rows 2 q and 2 q + 1
    shape = (n, n_q)
    words = HF.philox4x32_10(np.broadcast_to(lo[:, None], shape), np.broadcast_to(hi[:, None], shape),
                             np.broadcast_to(np.arange(n_q, dtype=np.uint64)[None, :], shape), np.full(shape, stream, dtype=np.uint64), k0, k1)
    u = np.stack([words[0], words[2]], axis=2).reshape(n, 2 * n_q)[:, :n_rows]      # u = w[a], a = 2 (r & 1)
    v = np.stack([words[1], words[3]], axis=2).reshape(n, 2 * n_q)[:, :n_rows]      # v = w[a + 1]
    flags = ((u * np.uint64(B)) >> _U32) == np.uint64(0)                            # u < 2^32, B < 2^31: no overflow
    flags[:, :1] = True                                                             # row 0 always restarts
    start = ((v * np.uint64(H)) >> _U32).astype(np.int64)
    # row_r = the start drawn at the last restart at or before r, plus the rows walked since, mod H: the recurrence unrolled
    r = np.broadcast_to(np.arange(n_rows, dtype=np.int64)[None, :], (n, n_rows))
    last = np.maximum.accumulate(np.where(flags, r, 0), axis=1)
    rows = (np.take_along_axis(start, last, axis=1) + (r - last)) % int(H)
    return (rows, flags) if restarts else rows


def cohort_rows(path_begin: int, n: int, n_rows: int, H: int) -> np.ndarray:
    """[n, n_rows] int64: row_r = ((path mod H) + r) mod H, path = path_begin + i as a Python integer."""
    start = np.array([(int(path_begin) + i) % int(H) for i in range(int(n))], dtype=np.int64)
    return (start[:, None] + np.arange(int(n_rows), dtype=np.int64)[None, :]) % int(H)


def rows_of(scheme: int, seed: int, stream: int, path_begin: int, n: int, n_rows: int, H: int, B: int) -> np.ndarray:
    if scheme == STATIONARY:
        return stationary_rows(seed, stream, path_begin, n, n_rows, H, B)
    if scheme == COHORTS:
        return cohort_rows(path_begin, n, n_rows, H)
    assert scheme == BLOCK, scheme
    return HF.history_rows(seed, stream, path_begin, n, n_rows, H, B)


def gathered(O, scn, table, B, scheme, wm=None, n=None, begin=None):
    """[n, shock_rows, 3]: the rows the plan's launch reads, as an `injected_shocks` block."""
    wm = scn.wm if wm is None else int(wm)
    n = scn.n if n is None else int(n)
    begin = scn.begin if begin is None else int(begin)
    rows = int(O.query_sizes(scn.params(), wm).shock_rows)
    return np.ascontiguousarray(np.asarray(table)[rows_of(scheme, scn.seed, scn.stream, begin, n, rows, len(table), B)])


_RUNS = {}


def oracle_run_scheme(O, scn, table, B, scheme, wm=None, n=None, trajectories=True, **over):
    """The oracle's `run_batch` of plan `scn` on the history stream under `scheme`: the gathered rows injected (cached per
    table, block and scheme)."""
    wm = scn.wm if wm is None else int(wm)
    n = scn.n if n is None else int(n)
    key = (int(scheme), scn.cls, scn.index, scn.seed, scn.stream, scn.begin, scn.cfgd["monthly_expenses"], n, wm, np.asarray(table).tobytes(), int(B),
           tuple(sorted((k, repr(v)) for k, v in over.items())))
    hit = _RUNS.get(key)
    if hit is None or (trajectories and "trajectory" not in hit):
        hit = O.run_batch(scn.params(**over), 0, scn.stream, 0, n, wm, injected_shocks=gathered(O, scn, table, B, scheme, wm, n),
                          want_trajectories=trajectories)
        _RUNS[key] = hit
    return hit
