"""The one rule by which a row of an in-kernel yearly table is compared with np.histogram of the ORACLE's row.

The kernel's values and the oracle's differ within the path tolerance, so an entry that lies within 1e-8 (relative,
``max(1, |edge|)``) of a bin edge may sit in the neighbouring bin on the device: a row that is not equal cell for cell may
move at most 2 x (its entries that near an edge), and holds each of its entries once.

The edge at 0.  `engine.default_year_edges()` and `engine.default_wr_edges()` start at ``edges[0] == 0.0``, and a failed path's
balance and a year without a withdrawal are exactly 0.0.  Counted as "near an edge", every such zero bought two moves that
nothing can spend: no value of the oracle or of the kernel is below zero, so an exact zero, or positive dust, lies in bin 0 on
both sides and the edge at 0 moves nothing.  For a table whose first edge is 0.0 the rule is therefore:

* cell 0 of the row (entries below ``edges[0]``) is 0 exactly;
* the edge at 0 is left out when the entries near an edge are counted.

`old_near` is the count with the edge at 0 kept: what the three call sites allowed before they called `check_row`.  It is here
for tests/test_bin_rule_cpu.py, which shows what it let through."""

from __future__ import annotations

import numpy as np

NEAR = 1e-8


def cells(row, edges) -> np.ndarray:
    """A row's table cells on `edges`: [below | np.histogram's bins | above], NaNs left out."""
    row = np.asarray(row, dtype=np.float64)
    row = row[~np.isnan(row)]
    return np.concatenate(([np.count_nonzero(row < edges[0])], np.histogram(row, bins=edges)[0],
                           [np.count_nonzero(row > edges[-1])])).astype(np.int64)


def _near(row, edges) -> int:
    if row.size == 0 or edges.size == 0:
        return 0
    return int(np.count_nonzero(np.min(np.abs(row[:, None] - edges[None, :]) - NEAR * np.maximum(1.0, np.abs(edges))[None, :], axis=1) <= 0))


def zero_edge(edges) -> bool:
    return float(edges[0]) == 0.0


def near_an_edge(row, edges) -> int:
    """Entries of `row` (NaNs left out) within 1e-8 of an edge that can move them: every edge but a first edge at 0.0."""
    row = np.asarray(row, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    return _near(row[~np.isnan(row)], edges[1:] if zero_edge(edges) else edges)


def old_near(row, edges) -> int:
    """The count with a first edge at 0.0 kept (the earlier rule): every exact zero of the row is in it."""
    row = np.asarray(row, dtype=np.float64)
    return _near(row[~np.isnan(row)], np.asarray(edges, dtype=np.float64))


def row_verdict(got, row, edges):
    """(moved, near, what is wrong or None) of table row `got` against the oracle's `row` on `edges`."""
    row = np.asarray(row, dtype=np.float64)
    row = row[~np.isnan(row)]
    edges = np.asarray(edges, dtype=np.float64)
    got = np.asarray(got).astype(np.int64).reshape(-1)
    exp = cells(row, edges)
    if got.shape != exp.shape:
        return 0, 0, f"{got.shape[0]} cells for {exp.shape[0]}"
    if int(got.sum()) != row.size:
        return 0, 0, f"the row holds {int(got.sum())} entries, the oracle's {row.size}"
    if zero_edge(edges) and int(got[0]) != 0:
        return 0, 0, f"{int(got[0])} entries below the edge at 0"
    moved = int(np.abs(got - exp).sum())
    if moved == 0:
        return 0, 0, None
    near = near_an_edge(row, edges)
    if moved > 2 * near:
        dist = np.sort(np.min(np.abs(row[:, None] - edges[None, :]) / np.maximum(1.0, np.abs(edges))[None, :], axis=1))[:4].tolist() if row.size else []
        return moved, near, f"{moved} moved, {near} near an edge (the edge at 0 apart); smallest relative distances to any edge {dist}"
    return moved, near, None


def check_row(got, row, edges, what="") -> tuple:
    """Assert the rule on one row; returns (moved, near)."""
    moved, near, wrong = row_verdict(got, row, edges)
    assert wrong is None, (wrong, what)
    return moved, near
