"""Worker for tests/test_gpu_joint_outcomes.py: one rank of a gloo group; both ranks share the box's GPU.  Each rank runs the
joint income probe of the claim-age table on its shard of the path range and must return the whole batch's matrix."""

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

#: a claim-age table of config.json's State Pension: early and small, the plan's own twice, late and large, none at all
CLAIMS = [{"start_at_age": 62.0, "monthly_amount_today": 2800.0}, {"start_at_age": 67.0, "monthly_amount_today": 4000.0},
          {"start_at_age": 67.0, "monthly_amount_today": 4000.0}, {"start_at_age": 70.0, "monthly_amount_today": 4960.0},
          {"monthly_amount_today": 0.0}]


def make_simulator():
    cfgd = dict(load_config_from_json(os.path.join(REPO, "scenarios", "config.json")), seed=11)
    sim = RetirementMonteCarloSimulator(Config(**cfgd))
    sim.use_final_seeds()
    return sim


def main():
    out_path = sys.argv[1]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    shards = []
    real = E.probe_income_joint

    def recording(params, seed, stream_id, path_begin, n_paths, *a, **k):
        shards.append((int(path_begin), int(n_paths)))
        return real(params, seed, stream_id, path_begin, n_paths, *a, **k)

    E.probe_income_joint = recording
    outcomes = make_simulator().joint_outcomes_by_income_options(240, "State Pension", CLAIMS, 5003)
    assert len(shards) == 1 and shards[0] == D.shard_range(5003, rank, world), shards
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump({"rank": rank, "joint": outcomes.joint.tolist(), "extremes": list(outcomes.extremes), "n_paths": outcomes.n_paths,
                   "probabilities": outcomes.probabilities.tolist(), "shard": list(shards[0])}, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
