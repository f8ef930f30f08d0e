"""Yearly bins against the count-only launch, and the trajectory-slab route they replace.

    python tools/year_bins_timing.py [out.json] [--reps 15] [--paths 1000000] [--slab-paths 10000000]

A/B at bench.py's headline shape (config.json, working_months = 233, --paths per launch), 64 and 256 bins: the count-only
launch with a final-balance histogram of that many bins against the yearly-bins launch with all four tables, interleaved
launch by launch in ONE process after warmup, HIP events, medians of --reps launches.  The tables of the yearly-bins launch are
checked for their row sums.  Then the slab route: a full-output launch plus `band_quantiles` at --slab-paths (0 = skip), with
its HBM footprint.  Prints one line per shape and writes every sample to out.json."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from monte_carlo_retirement_amd import Config, params_from_config  # noqa: E402
from monte_carlo_retirement_amd import aggregation as A  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKING_MONTHS = 233


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--paths", type=int, default=1_000_000)
    ap.add_argument("--slab-paths", type=int, default=10_000_000)
    args = ap.parse_args()
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        params = params_from_config(Config(**dict(json.load(fh), seed=12345)))
    n = args.paths
    res = {"device": torch.cuda.get_device_name(0), "scenario": "config.json", "working_months": WORKING_MONTHS, "paths": n,
           "reps": args.reps, "shapes": []}
    for n_bins in (64, 256):
        count = E.DeviceBatch(params, WORKING_MONTHS, n, want="count", hist_edges=E.default_year_edges(n_bins))
        bins = E.YearBinsBatch(params, WORKING_MONTHS, E.default_year_edges(n_bins), E.default_wr_edges(n_bins))
        for _ in range(3):
            count.launch(12345, 1, 0)
            bins.launch(12345, 1, 0, n)
        torch.cuda.synchronize()
        count.zero_counters()
        bins.zero()
        a, b = [], []
        for _ in range(args.reps):
            a.append(timed(lambda: count.launch(12345, 1, 0)))
            b.append(timed(lambda: bins.launch(12345, 1, 0, n)))
        host = bins.host()
        total = n * args.reps
        ok = (int(host["counters"][1]) == total and bool((host["trajectory_bins"].sum(axis=1) == total).all())
              and bool((host["real_trajectory_bins"].sum(axis=1) == total).all())
              and bool((host["wr_bins"].sum(axis=1) == host["wr_obs_counts"]).all())
              and int(host["final_success_bins"].sum()) == int(host["counters"][0]) == int(count.counters[0]))
        ma, mb = statistics.median(a), statistics.median(b)
        shape = {"n_bins": n_bins, "count_only_hist_ms": a, "year_bins_ms": b, "median_count_only_hist_ms": ma, "median_year_bins_ms": mb,
                 "ratio": mb / ma, "row_sums_ok": ok, "int64_words": int(bins.reduce_vec.numel())}
        res["shapes"].append(shape)
        print(f"{n_bins:4d} bins: count-only + histogram {ma:8.3f} ms | yearly bins (4 tables) {mb:8.3f} ms | ratio {mb / ma:.3f} | "
              f"row sums {'ok' if ok else 'WRONG'} | {bins.reduce_vec.numel() * 8 / 1024:.0f} KiB of integers", flush=True)
        del count, bins
    if args.slab_paths > 0:
        m = args.slab_paths
        torch.cuda.reset_peak_memory_stats()
        batch = E.DeviceBatch(params, WORKING_MONTHS, m, want="full")
        batch.launch(12345, 1, 0)
        A.band_quantiles(batch, m)                     # warm-up (scratch allocation)
        t_launch, t_bands = [], []
        for _ in range(3):
            t_launch.append(timed(lambda: batch.launch(12345, 1, 0)))
            t_bands.append(timed(lambda: A.band_quantiles(batch, m)))
        slab = {"paths": m, "full_output_launch_ms": t_launch, "band_quantiles_ms": t_bands,
                "median_total_ms": statistics.median(t_launch) + statistics.median(t_bands),
                "slab_bytes": int(batch.slab.numel() * 8), "peak_allocated_bytes": int(torch.cuda.max_memory_allocated()),
                "bytes_per_path": batch.slab.numel() * 8 / m}
        res["slab_route"] = slab
        print(f"slab route, {m} paths: launch {statistics.median(t_launch):.1f} ms + bands {statistics.median(t_bands):.1f} ms; "
              f"slab {slab['slab_bytes'] / 2**30:.2f} GiB ({slab['bytes_per_path']:.0f} B/path), peak {slab['peak_allocated_bytes'] / 2**30:.2f} GiB",
              flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
