"""Wall time of the host-buffer entry points (whichever library MCR_HIP_LIBRARY names), one JSON line."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from monte_carlo_retirement_amd import Config, params_from_config  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return {"median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1), "p90_us": round(ts[int(len(ts) * 0.9)], 1)}


def main():
    with open(os.path.join(REPO, "tests", "golden", "metric_10k_config_json.json")) as fh:
        meta = json.load(fh)
    p = params_from_config(Config(**meta["cfg"]))
    wm, n = meta["working_months"], int(meta["n_paths"])
    e, we = E.default_year_edges(64), E.default_wr_edges(64)
    out = {"library": os.environ.get("MCR_HIP_LIBRARY", "tree")}
    out["batch_10k_summary"] = timed(lambda: E.run_batch_host(p, meta["seed"], 1, 0, n, wm, want_trajectories=False), 200)
    out["batch_2048_full"] = timed(lambda: E.run_batch_host(p, 12345, 1, 0, 2048, wm), 200)
    out["batch_10k_summary_3shards"] = timed(lambda: E.run_batch_host(p, meta["seed"], 1, 0, n, wm, want_trajectories=False, devices=[0, 0, 0]), 100)
    out["year_bins_5003"] = timed(lambda: E.run_year_bins_host(p, 99, 1, 0, 5003, wm, edges=e, wr_edges=we), 200)
    out["year_bins_5003_3shards"] = timed(lambda: E.run_year_bins_host(p, 99, 1, 0, 5003, wm, edges=e, wr_edges=we, devices=[0, 0, 0]), 100)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
