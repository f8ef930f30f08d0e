#!/usr/bin/env python3
"""Count-only launch time of the spending-rule launch (mcr_run_rule_rng) beside the plain launch of the same block:
scenarios/config.json at 10^6 paths and 233 working months (833 months a path), the median of 20 event-timed launches after
warm-up, each median taken `--repeats` times in a process of its own (the spread of those medians is the run-to-run noise).

    python tools/rule_bench.py [out.json] [--parent-library PATH/libmcr_hip.so] [--reps 20] [--repeats 5]

Rows:
  rule_neutral      the rule launch under the neutral rule (cut = raise = 0): the plain launch's arithmetic on the generic tax
                    mask, plus the year's decision, four ballots and at most four atomics a wave and year
  rule_symmetric    the rule launch under a rule that fires (1.2, 0.8, 0.10, 0.10, 0.5, 1.5)
  plain_whole_path  the plain whole-path count-only launch (MCR_K1_SCREEN=0, MCR_K1_SEGMENTS=0: one launch of the lean kernel of
                    the block's tax mask and forms), from --parent-library when given (the parent commit's build, loaded
                    through MCR_HIP_LIBRARY), else from this build
  plain_default     the same library's count-only launch as callers get it (at this size: the screened route)
Nothing is judged: the rule launch has no earlier figure to be held to.  A child process measures the rows asked of it."""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_PATHS, WM, SEED, STREAM = 1_000_000, 233, 12345, 1
WARMUP = 3
RULES = {"rule_neutral": (1.0, 1.0, 0.0, 0.0, 1.0, 1.0), "rule_symmetric": (1.2, 0.8, 0.10, 0.10, 0.5, 1.5)}


def timed(launch, reps: int):
    import torch

    for _ in range(WARMUP):
        launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def child(reps: int) -> int:
    from monte_carlo_retirement_amd import Config, params_from_config
    from monte_carlo_retirement_amd import _native as N
    from monte_carlo_retirement_amd import engine as E

    p = params_from_config(Config(**json.load(open(os.path.join(REPO, "scenarios", "config.json")))))
    rows = os.environ["RULE_BENCH_ROWS"].split(",")
    out = {}
    for name in rows:
        if name in RULES:
            rule = N.McrSpendingRule(*RULES[name])
            last = {}

            def launch():
                last["res"] = E.run_rule(p, SEED, STREAM, 0, N_PATHS, WM, rule)

            out[name] = timed(launch, reps)
            counts = last["res"]["counts"].cpu().numpy()
            out[name]["successes"] = int(counts[0])
            out[name]["cut_path_years"] = int(counts[2:].reshape(-1, 4)[:, 1].sum())
        else:
            b = E.DeviceBatch(p, WM, N_PATHS, want="count")

            def launch():
                b.zero_counters()
                b.launch(SEED, STREAM, 0)

            out[name] = timed(launch, reps)
            out[name]["successes"] = int(b.counters[0].item())
    print(json.dumps(out), flush=True)
    return 0


def run_child(reps: int, rows, library=None, env_extra=None):
    env = dict(os.environ)
    for k in ("MCR_HIP_LIBRARY", "MCR_K1_SCREEN", "MCR_K1_SEGMENTS"):
        env.pop(k, None)
    if library:
        env["MCR_HIP_LIBRARY"] = library
    env["RULE_BENCH_ROWS"] = ",".join(rows)
    env.update(env_extra or {})
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
    runs = {name: [] for name in ("rule_neutral", "rule_symmetric", "plain_whole_path", "plain_default")}
    for _ in range(repeats):
        for name, row in run_child(reps, list(RULES)).items():
            runs[name].append(row)
        runs["plain_whole_path"].append(run_child(reps, ["plain_whole_path"], parent, {"MCR_K1_SCREEN": "0", "MCR_K1_SEGMENTS": "0"})["plain_whole_path"])
        runs["plain_default"].append(run_child(reps, ["plain_default"], parent)["plain_default"])
    summary = {}
    for name, rows in runs.items():
        medians = [r["median_ms"] for r in rows]
        summary[name] = {"median_ms": statistics.median(medians), "medians_ms": medians, "spread_ms": max(medians) - min(medians),
                         "successes": rows[0]["successes"], **({"cut_path_years": rows[0]["cut_path_years"]} if "cut_path_years" in rows[0] else {})}
        src = ("parent library" if parent else "this build") if name.startswith("plain") else "this build"
        print(f"{name:>17} ({src}), {N_PATHS} paths count-only: median {summary[name]['median_ms']:.3f} ms, medians "
              f"{[round(m, 3) for m in medians]}, spread {summary[name]['spread_ms']:.3f} ms, successes {summary[name]['successes']}", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"n_paths": N_PATHS, "working_months": WM, "reps": reps, "repeats": repeats,
                       "plain_library": "parent" if parent else "this build", "rows": summary}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
