"""Worker for tests/test_gpu_year_bins.py: one rank of a two-rank gloo group; both ranks share the box's GPU.  Runs
`run_sharded_year_bins` over 10 007 jorge.json paths and reports the summed vector and how many collectives ran."""

from __future__ import annotations

import json
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from monte_carlo_retirement_amd import Config, params_from_config  # noqa: E402
from monte_carlo_retirement_amd import distributed as D  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402


def main():
    out_path = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    with open(os.path.join(REPO, "scenarios", "jorge.json")) as fh:
        cfg = Config(**dict(json.load(fh), seed=12345, equity_inflation_correlation=0.3))
    calls = []
    real = dist.all_reduce

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    dist.all_reduce = counting
    try:
        res = D.run_sharded_year_bins(params_from_config(cfg), 2024, 1, 10_007, 75, E.default_year_edges(64), E.default_wr_edges(64))
    finally:
        dist.all_reduce = real
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump({"rank": rank, "vector": res["vector"].tolist(), "exchange": res["exchange"], "collectives": len(calls)}, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
