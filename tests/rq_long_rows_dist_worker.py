"""Worker for tests/test_gpu_band_shapes.py::test_long_rows_sharded_over_two_ranks: one rank of a gloo group (all ranks
share the box's GPU) holding its shard of rows that are longer than 2^24 entries IN TOTAL and shorter than that PER RANK
— `mcr_row_quantiles_sharded` then takes its sub-bin width from n_total and sizes its candidate buffers from n_local.
Also the home of `long_rows`, the slab both that test and the single-GPU long-row tests draw."""

from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

LONG_N = (1 << 24) + 71          # odd, above the 2^24 switch to 10-bit sub-histograms
LONG_SEED = 20260224
NINE = (0.01, 0.05, 0.10, 0.25, 0.50, 0.75, 0.90, 0.95, 0.99)      # the response document's final-balance percentiles
SHARDED_ROWS = (0, 1, 2, 4)


def long_rows(n: int = LONG_N, seed: int = LONG_SEED) -> np.ndarray:
    """[5, n]: continuous | continuous with 20 % NaN | constant | every magnitude and both signs (its bounds do not fit the
    slab pass's bucket table) | 65 % exact zeros plus a continuous tail (a giant tie: the radix passes)."""
    rng = np.random.default_rng(seed)
    rows = np.empty((5, n))
    rows[0] = rng.lognormal(14, 1.2, n)
    rows[1] = np.where(rng.random(n) < 0.2, np.nan, rng.normal(4.0, 1.5, n))
    rows[2] = 1.0e6
    rows[3] = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 9, n)
    rows[4] = np.where(rng.random(n) < 0.65, 0.0, rng.lognormal(10, 2, n))
    return rows


def main():
    import torch
    import torch.distributed as dist

    sys.path.insert(0, REPO)
    from monte_carlo_retirement_amd import aggregation as A
    from monte_carlo_retirement_amd import distributed as D

    out_path = sys.argv[1]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    slab = long_rows()[list(SHARDED_ROWS)]
    begin, count = D.shard_range(LONG_N, rank, world)
    assert count < (1 << 24) < LONG_N
    local = torch.full((len(SHARDED_ROWS), (count + 63) // 64 * 64), 7.0, dtype=torch.float64, device="cuda")
    local[:, :count] = torch.as_tensor(np.ascontiguousarray(slab[:, begin:begin + count]), device="cuda")
    del slab
    res = {}
    for name, qs in (("seven", A.TRAJECTORY_QUANTILES), ("nine", NINE)):
        q, counts = D.sharded_row_quantiles(local, count, qs)
        res[f"bracket_{name}_q"], res[f"bracket_{name}_counts"], res[f"bracket_{name}_fallback"] = q, counts, A.last_fallback_rows()
    os.environ["MCR_RQ_SHARDED_BRACKET_MIN_N"] = str(2**40)          # the stepwise radix select, digit histograms summed per pass
    for name, qs in (("seven", A.TRAJECTORY_QUANTILES), ("nine", NINE)):
        q, counts = D.sharded_row_quantiles(local, count, qs)
        res[f"radix_{name}_q"], res[f"radix_{name}_counts"] = q, counts
    del os.environ["MCR_RQ_SHARDED_BRACKET_MIN_N"]
    np.savez(f"{out_path}.{rank}.npz", **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
