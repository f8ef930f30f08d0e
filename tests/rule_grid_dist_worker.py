"""Worker for tests/test_gpu_rule_grid_probe.py: one rank of a gloo group; both ranks share the box's GPU.  Each rank runs the
grid under a spending rule on its share of the work and must hold the whole batch's matrix: sharded by path range (every rank
probes every row on its half of the paths), and split by candidate (each rank probes every other row over the whole range)."""

from __future__ import annotations

import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import spending_rule_model as M  # noqa: E402
from monte_carlo_retirement_amd import Config  # noqa: E402
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator  # noqa: E402
from monte_carlo_retirement_amd.spending_rules import SpendingRule  # noqa: E402

N_PATHS = 1203
MONTHS = [120, 0, 7, 121, 60]
LEVELS = [M.LEVELS["realized", 7]["symmetric"], M.LEVELS["realized", 120]["symmetric"], 0.0]
RULE = M.RULES["symmetric"]


def make_simulator():
    sim = RetirementMonteCarloSimulator(Config(**M.plan_config("realized", REPO)), main_seed_override=M.SEED)
    sim.use_final_seeds()
    return sim


def matrices(sim):
    """What every rank must agree on: the matrix sharded by path range, and split by candidate."""
    rule = SpendingRule(*RULE)
    sim.shard_min_paths = 0            # shard by path range at any size
    by_range = sim.success_probability_grid_with_rule(MONTHS, rule, LEVELS, N_PATHS)
    sim.shard_min_paths = 1 << 40      # never: split by candidate (row)
    by_row = sim.success_probability_grid_with_rule(MONTHS, rule, LEVELS, N_PATHS)
    return {"by_path_range": by_range.tolist(), "by_candidate": by_row.tolist()}


def main():
    import torch
    import torch.distributed as dist

    from monte_carlo_retirement_amd import engine as E

    out_path = sys.argv[1]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    calls = []
    real = E.probe_rule_grid

    def recording(params, seed, stream_id, path_begin, n_paths, working_months, levels_2d, rule, **k):
        calls.append((int(path_begin), int(n_paths), [int(m) for m in working_months]))
        return real(params, seed, stream_id, path_begin, n_paths, working_months, levels_2d, rule, **k)

    E.probe_rule_grid = recording
    docs = matrices(make_simulator())
    assert len(calls) == 2, calls
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump({"rank": rank, "matrices": docs, "by_path_range": list(calls[0]), "by_candidate": list(calls[1])}, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
