"""Worker for tests/test_gpu_option_outcomes.py: one rank of a gloo group; both ranks share the box's GPU.  Each rank runs the
income outcomes probe of the claim-age table on its shard of the path range and must return the whole batch's outcomes."""

from __future__ import annotations

import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from joint_dist_worker import CLAIMS, make_simulator  # noqa: E402,F401

N_PATHS = 5003


def outcomes_document(o):
    """An `OptionOutcomes` as JSON-able values, every number kept exactly (floats as their hex strings)."""
    return {"n_paths": o.n_paths, "successes": o.successes.tolist(), "ruin_months": o.ruin_months.tolist(), "cohort": o.cohort.tolist(),
            "quantiles": list(o.quantiles), "final_quantiles": [[float(x).hex() for x in row] for row in o.final_quantiles],
            "retirement_age": o.retirement_age, "probabilities": o.probabilities.tolist(),
            "rows": [o.row(k) for k in range(len(o))]}


def main():
    import torch
    import torch.distributed as dist

    from monte_carlo_retirement_amd import distributed as D
    from monte_carlo_retirement_amd import engine as E

    out_path = sys.argv[1]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    shards = []
    real = E.probe_income_outcomes

    def recording(params, seed, stream_id, path_begin, n_paths, *a, **k):
        shards.append((int(path_begin), int(n_paths)))
        return real(params, seed, stream_id, path_begin, n_paths, *a, **k)

    E.probe_income_outcomes = recording
    outcomes = make_simulator().option_outcomes_by_income_options(240, "State Pension", CLAIMS, N_PATHS)
    assert len(shards) == 1 and shards[0] == D.shard_range(N_PATHS, rank, world), shards
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump({"rank": rank, "outcomes": outcomes_document(outcomes), "shard": list(shards[0])}, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
