#!/usr/bin/env python3
"""Count-only launch time of the history stream (rng="history") beside the engine's own streams, scenarios/config.json at
10^6 paths and 233 working months (833 months a path): the median of 20 event-timed launches after warm-up, per stream.

    python tools/history_bench.py [out.json] [--parent-library PATH/libmcr_hip.so] [--reps 20] [--repeats 5]

The yardstick is the PARENT commit's library (built from the parent, loaded through MCR_HIP_LIBRARY in child processes):
its Philox launch and its own fixed-block history launches (the parent reads a prefix of today's descriptor, so they are
timed through this tree's Python).  Each median is taken `--repeats` times, each in a process of its own, and the spread of
those medians is the run-to-run noise this build is judged against:

  * the fixed-block rows (history_600, history_2048) against the parent's SAME row: median + spread — the scheme branch must
    not slow the rule that was there;
  * the stationary rows against the parent's Philox row: median + spread — a third of the generator work and no
    transcendental per month, so a slower launch means the cursor has the wrong shape;
  * the cohort row is recorded: it has no generator at all.

Without --parent-library the yardstick is this build's own launches (the fingerprint comparison of tools/isa_fingerprint.py
says whether those are the same kernels).  A child process measures every stream asked of it: one JSON line."""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_PATHS, WM, SEED, STREAM, BLOCK = 1_000_000, 233, 12345, 1, 12
WARMUP = 3


def record(months: int):
    """A standardised record of independent normal months: the config's own distribution, so the paths fail about as often
    as on the Philox stream and the launches do comparable work."""
    import numpy as np

    z = np.random.default_rng(months).standard_normal((months, 3))
    return (z - z.mean(axis=0)) / z.std(axis=0)


def child(reps: int) -> int:
    import torch

    from monte_carlo_retirement_amd import Config, params_from_config
    from monte_carlo_retirement_amd import _native as N
    from monte_carlo_retirement_amd import engine as E

    p = params_from_config(Config(**json.load(open(os.path.join(REPO, "scenarios", "config.json")))))
    streams = {"philox": SEED, "numpy": N.numpy_rng(SEED)}
    if hasattr(N, "history_rng"):
        streams["history_600"] = N.history_rng(SEED, record(600), BLOCK)
        streams["history_2048"] = N.history_rng(SEED, record(2048), BLOCK)
    if hasattr(N, "MCR_HISTORY_STATIONARY"):       # (rows a parent library is never asked for: it reads no scheme)
        streams["history_600_stationary"] = N.history_rng(SEED, record(600), BLOCK, N.MCR_HISTORY_STATIONARY)
        streams["history_2048_stationary"] = N.history_rng(SEED, record(2048), BLOCK, N.MCR_HISTORY_STATIONARY)
        streams["history_600_cohorts"] = N.history_rng(SEED, record(600), BLOCK, N.MCR_HISTORY_COHORTS)
    only = os.environ.get("HISTORY_BENCH_ONLY")
    out = {}
    for name, rng in streams.items():
        if only and name not in only.split(","):
            continue
        b = E.DeviceBatch(p, WM, N_PATHS, want="count")
        for _ in range(WARMUP):
            b.launch(rng, STREAM, 0)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            b.zero_counters()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.launch(rng, STREAM, 0)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        out[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "successes": int(b.counters[0].item())}
    print(json.dumps(out), flush=True)
    return 0


def run_child(reps: int, library=None, only=None):
    env = dict(os.environ)
    env.pop("MCR_HIP_LIBRARY", None)
    env.pop("HISTORY_BENCH_ONLY", None)
    if library:
        env["MCR_HIP_LIBRARY"] = library
    if only:
        env["HISTORY_BENCH_ONLY"] = only
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({library or 'this build'}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main() -> int:
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 20
    if "--child" in args:
        return child(reps)
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 5
    parent = os.path.abspath(args[args.index("--parent-library") + 1]) if "--parent-library" in args else None
    out_path = next((a for a in args if a.endswith(".json")), None)
    yard_rows = ("philox", "history_600", "history_2048")
    yard = [run_child(reps, parent, ",".join(yard_rows)) for _ in range(repeats)]
    bounds = {}
    for name in yard_rows:
        medians = [y[name]["median_ms"] for y in yard]
        spread = max(medians) - min(medians)
        bounds[name] = {"medians_ms": medians, "spread_ms": spread, "bound_ms": statistics.median(medians) + spread}
        print(f"yardstick ({'parent library' if parent else 'this build'}), {name:>12} count-only, {N_PATHS} paths: medians {[round(m, 3) for m in medians]} ms, "
              f"spread {spread:.3f} ms", flush=True)
    own = run_child(reps)
    ok = True
    for name, row in own.items():
        against = name if name in ("history_600", "history_2048") else "philox" if name.endswith("_stationary") else None
        verdict = ""
        if against:
            row["bound_ms"], row["bound_row"] = bounds[against]["bound_ms"], against
            row["within_bound"] = row["median_ms"] <= row["bound_ms"]
            ok = ok and row["within_bound"]
            verdict = f"; {'within' if row['within_bound'] else 'NOT within'} the yardstick's {against} median + spread = {row['bound_ms']:.3f} ms"
        print(f"this build, {name:>23}: median {row['median_ms']:.3f} ms (min {row['min_ms']:.3f}, max {row['max_ms']:.3f}), successes {row['successes']}{verdict}",
              flush=True)
    print(f"the history launches {'are' if ok else 'are NOT'} within their bounds", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"n_paths": N_PATHS, "working_months": WM, "block_months": BLOCK, "reps": reps, "yardstick_library": "parent" if parent else "this build",
                       "yardstick": yard, "yardstick_bounds": bounds, "this_build": own, "within_bound": ok}, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
