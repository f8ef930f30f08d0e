"""Worker for tests/test_gpu_allocation_simulator.py: one rank of a gloo group; both ranks share the box's GPU.  Each rank runs
`compare_allocations(paired=True, outcomes=True)` on its shard of the path range and must return the whole batch's document."""

from __future__ import annotations

import json
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from monte_carlo_retirement_amd import Config, load_config_from_json  # noqa: E402
from monte_carlo_retirement_amd import distributed as D  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator  # noqa: E402

WM = 240
N_PATHS = 5003
#: the plan's own split, both ends, a duplicate, and an option whose spending differs as well
SPLITS = [0.0, 0.3, 0.6, 0.6, 1.0, {"allocation_inv1_pct": 0.45, "monthly_expenses": 7000.0}]


def make_simulator(rng="philox", **over):
    cfgd = dict(load_config_from_json(os.path.join(REPO, "scenarios", "config.json")), seed=11, **over)
    sim = RetirementMonteCarloSimulator(Config(**cfgd), rng=rng)
    sim.use_final_seeds()
    return sim


def main():
    out_path = sys.argv[1]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    shards = []

    def recording(real):
        def call(params, seed, stream_id, path_begin, n_paths, *a, **k):
            shards.append((int(path_begin), int(n_paths)))
            return real(params, seed, stream_id, path_begin, n_paths, *a, **k)
        return call

    E.probe_allocations_joint = recording(E.probe_allocations_joint)
    E.probe_allocations_outcomes = recording(E.probe_allocations_outcomes)
    doc = make_simulator().compare_allocations(WM, SPLITS, N_PATHS, paired=True, outcomes=True)
    assert shards == [D.shard_range(N_PATHS, rank, world)] * 2, shards      # the joint probe, then the outcomes probe
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump({"rank": rank, "document": doc, "shard": list(shards[0])}, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
