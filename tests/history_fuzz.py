"""The history stream (include/mcr.h: MCR_RNG_HISTORY) restated on the CPU, a synthetic record, and the oracle's answer to a
plan on that stream.

`history_rows` is the rule of the header in NumPy uint64 arithmetic, with a Philox4x32-10 of its own (held to the oracle's
by tests/test_history_cpu.py).  The oracle has no such stream and needs none: it takes the gathered rows through
`injected_shocks`, which is what the stream means."""

from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
RECORD_SEED, RECORD_MONTHS = 20261019, 600


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of counters: uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def history_rows(seed: int, stream: int, path_begin: int, n: int, n_rows: int, H: int, B: int) -> np.ndarray:
    """[n, n_rows] int64: the row of the record that shock row r of global path path_begin + i reads."""
    shape = (int(n), int(n_rows))
    path = np.broadcast_to((np.arange(n, dtype=np.uint64) + np.uint64(path_begin))[:, None], shape)
    r = np.broadcast_to(np.arange(n_rows, dtype=np.uint64)[None, :], shape)
    k, j = r // np.uint64(B), r % np.uint64(B)
    words = philox4x32_10(path & M32, path >> np.uint64(32), k >> np.uint64(2), np.full(shape, stream, dtype=np.uint64),
                          int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    x = np.choose((k & np.uint64(3)).astype(np.int64), words)
    s = (x * np.uint64(H)) >> np.uint64(32)          # x < 2^32, H <= 2048: no overflow
    return ((s + j) % np.uint64(H)).astype(np.int64)


_RECORD = {}


def synthetic_record(H: int = RECORD_MONTHS) -> np.ndarray:
    """Z[H][3]: Student-t(5) innovations scaled to unit variance, an AR(1) of coefficient 0.3 per series, inflation mixed 0.3
    with equity, every column standardised.  Fat tails, clustering within a series and co-movement across two: what a block
    keeps and an i.i.d. draw loses."""
    if H not in _RECORD:
        rng = np.random.default_rng(RECORD_SEED)
        e = rng.standard_t(5, size=(H, 3)) / np.sqrt(5.0 / 3.0)
        x = np.zeros((H, 3))
        for t in range(H):
            x[t] = (0.3 * x[t - 1] if t else 0.0) + e[t]
        x[:, 1] = 0.3 * x[:, 0] + x[:, 1]
        sd = x.std(axis=0)
        z = (x - x.mean(axis=0)) / np.where(sd > 0.0, sd, 1.0)
        z.setflags(write=False)
        _RECORD[H] = z
    return _RECORD[H]


_RUNS = {}


def gathered(O, scn, table, B, wm=None, n=None, begin=None):
    """[n, shock_rows, 3]: the rows the plan's launch reads, as an `injected_shocks` block."""
    wm = scn.wm if wm is None else int(wm)
    n = scn.n if n is None else int(n)
    begin = scn.begin if begin is None else int(begin)
    rows = int(O.query_sizes(scn.params(), wm).shock_rows)
    return np.ascontiguousarray(np.asarray(table)[history_rows(scn.seed, scn.stream, begin, n, rows, len(table), B)])


def oracle_run_history(O, scn, table, B, wm=None, n=None, trajectories=True, **over):
    """The oracle's `run_batch` of plan `scn` on the history stream: the gathered rows injected (cached per table and block)."""
    wm = scn.wm if wm is None else int(wm)
    n = scn.n if n is None else int(n)
    key = (scn.cls, scn.index, scn.seed, scn.stream, scn.begin, scn.cfgd["monthly_expenses"], n, wm, np.asarray(table).tobytes(), int(B),
           tuple(sorted((k, repr(v)) for k, v in over.items())))
    hit = _RUNS.get(key)
    if hit is None or (trajectories and "trajectory" not in hit):
        hit = O.run_batch(scn.params(**over), 0, scn.stream, 0, n, wm, injected_shocks=gathered(O, scn, table, B, wm, n), want_trajectories=trajectories)
        _RUNS[key] = hit
    return hit
