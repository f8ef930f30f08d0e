"""Worker for tests/test_gpu_glide_run_simulator.py: one rank of a two-rank gloo group; both ranks share the box's GPU.  Runs
`run_sharded_year_bins` under a glide path over its shard of the path range and reports the summed vector — the whole batch's
tables — and how many collectives ran."""

from __future__ import annotations

import json
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from monte_carlo_retirement_amd import Config, params_from_config  # noqa: E402
from monte_carlo_retirement_amd import distributed as D  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402
from monte_carlo_retirement_amd.allocation import GlidePath  # noqa: E402

PLAN, WM, LEVEL, N_PATHS = "streams", 120, "neutral", 5003
GLIDE = GlidePath.around_retirement(WM, 0.9, 0.5, 0.3, 8, 10)


def main():
    import spending_rule_model as M

    out_path = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    cfg = Config(**dict(M.plan_config(PLAN, REPO, WM), monthly_expenses=M.LEVELS[PLAN, WM][LEVEL]))
    calls = []
    real = dist.all_reduce

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    dist.all_reduce = counting
    try:
        res = D.run_sharded_year_bins(params_from_config(cfg), M.SEED, M.STREAM, N_PATHS, WM, E.default_year_edges(64), E.default_wr_edges(64),
                                      glide_path=GLIDE)
    finally:
        dist.all_reduce = real
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump({"rank": rank, "vector": res["vector"].tolist(), "exchange": res["exchange"], "collectives": len(calls),
                   "shard": list(res["shard"])}, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
