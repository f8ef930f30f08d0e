"""Worker for tests/test_grid_search_cpu.py: one rank of a gloo process group on the CPU.

The local "kernel" is a deterministic stub that counts successes of a path range from integer arithmetic every rank can
reproduce; what is under test is the grid's multi-rank layer: `distributed.probe_candidates` with one candidate per grid
row and ``2 L`` counters each, under the lockstep search."""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch.distributed as dist

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from monte_carlo_retirement_amd import distributed as D  # noqa: E402
from monte_carlo_retirement_amd.spending import search_maximum_expenses_many  # noqa: E402


def share(month, x):   # success share at a month and spending level
    return max(0.0, min(1.0, 1.0 - (int(x * 100) * 7919 % 1009) / 20000.0 - x / (30.0 * (100 + month))))


def main():
    n_total, shard_min, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    calls = []

    def grid(months, levels_2d):
        L = len(levels_2d[0])

        def probe(path_begin, count, idx):
            calls.append((path_begin, count, list(idx)))
            return np.array([[[int(round(share(months[i], x) * (path_begin + count))) - int(round(share(months[i], x) * path_begin)),
                               count] for x in levels_2d[i]] for i in idx], dtype=np.int64)

        counts = D.probe_candidates(list(range(len(months))), n_total, shard_min, probe, width=2 * L)
        return counts.reshape(len(months), L, 2)

    months = [120, 180, 240, 300, 360]
    levels = [100.0, 2000.0, 3500.5, 7000.0]
    g = grid(months, [levels] * len(months))

    def probe_rows(rows, levels_2d):
        c = grid([months[i] for i in rows], levels_2d)
        return (c[:, :, 0].astype(np.float64) / np.float64(n_total) * 100.0).tolist()

    frontier = search_maximum_expenses_many(probe_rows, 80.0, [100.0] * len(months), levels_per_call=15, working_months=months)
    with open(out + str(rank), "w") as fh:
        json.dump({"grid": g.tolist(), "months": months, "levels": levels,
                   "share": [[share(m, x) for x in levels] for m in months], "frontier": frontier, "calls": calls}, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
