#!/usr/bin/env python3
"""Launch time of the yearly-bins launch under a spending rule (mcr_run_rule_year_bins_rng) beside the launches it combines:
scenarios/config.json at 10^6 paths and 233 working months (833 months a path), 64 + 64 + 64 bins (balance, withdrawal rate,
multiplier), the median of 20 event-timed launches after warm-up, each median taken `--repeats` times in a process of its own
(the spread of those medians is the run-to-run noise).

    python tools/rule_year_bins_timing.py [out.json] [--parent-library PATH/libmcr_hip.so] [--reps 20] [--repeats 5]

Rows:
  rule_bins_neutral / rule_bins_symmetric    (a) the new launch, all four tables, year counts and multiplier bins, this build
  plain_year_bins                            (b) the plain yearly-bins launch (mcr_run_year_bins_rng), all four tables
  rule_count_neutral / rule_count_symmetric  (c) the count-only rule launch (mcr_run_rule_rng) with its year counts
  plain_whole_path                           the plain whole-path count-only launch (MCR_K1_SCREEN=0, MCR_K1_SEGMENTS=0)
(b), (c) and the last row come from --parent-library when given (the parent commit's build, loaded through MCR_HIP_LIBRARY),
else from this build.  Printed with them: (a) / (b), (a) / (c), and the two increments the form adds, (a) - (c) under each rule
against (b) - plain_whole_path.  Nothing is judged: the launch has no earlier figure to be held to.  The new launch's row sums
are checked.  A child process measures the rows asked of it."""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_PATHS, WM, SEED, STREAM, N_BINS = 1_000_000, 233, 12345, 1, 64
WARMUP = 3
RULES = {"neutral": (1.0, 1.0, 0.0, 0.0, 1.0, 1.0), "symmetric": (1.2, 0.8, 0.10, 0.10, 0.5, 1.5)}
ROWS = ("rule_bins_neutral", "rule_bins_symmetric", "plain_year_bins", "rule_count_neutral", "rule_count_symmetric", "plain_whole_path")


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
    import numpy as np

    from monte_carlo_retirement_amd import Config, params_from_config
    from monte_carlo_retirement_amd import _native as N
    from monte_carlo_retirement_amd import engine as E

    p = params_from_config(Config(**json.load(open(os.path.join(REPO, "scenarios", "config.json")))))
    edges, wr_edges = E.default_year_edges(N_BINS), E.default_wr_edges(N_BINS)
    out = {}
    for name in os.environ["RULE_YEAR_BINS_ROWS"].split(","):
        kind, _, rname = name.rpartition("_")
        if kind == "rule_bins":
            rule = N.McrSpendingRule(*RULES[rname])
            b = E.YearBinsBatch(p, WM, edges, wr_edges, rule=rule, m_edges=np.linspace(0.5, 1.5, N_BINS + 1))
            out[name] = timed(lambda: b.launch(SEED, STREAM, 0, N_PATHS), reps)
            h = b.host()
            total = N_PATHS * (reps + WARMUP)
            out[name]["row_sums_ok"] = bool(
                int(h["counters"][1]) == total and (h["trajectory_bins"].sum(axis=1) == total).all()
                and (h["wr_bins"].sum(axis=1) == h["wr_obs_counts"]).all() and int(h["final_success_bins"].sum()) == int(h["counters"][0])
                and (h["multiplier_bins"].sum(axis=1) == h["rule_year_counts"][:, N.MCR_RULE_ALIVE]).all())
            out[name]["successes"] = int(h["counters"][0]) // (reps + WARMUP)
        elif name == "plain_year_bins":
            b = E.YearBinsBatch(p, WM, edges, wr_edges)
            out[name] = timed(lambda: b.launch(SEED, STREAM, 0, N_PATHS), reps)
            out[name]["successes"] = int(b.counters[0].item()) // (reps + WARMUP)
        elif kind == "rule_count":
            rule = N.McrSpendingRule(*RULES[rname])
            last = {}

            def launch():
                last["res"] = E.run_rule(p, SEED, STREAM, 0, N_PATHS, WM, rule)

            out[name] = timed(launch, reps)
            out[name]["successes"] = int(last["res"]["counts"][0].item())
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
    env["RULE_YEAR_BINS_ROWS"] = ",".join(rows)
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
    runs = {name: [] for name in ROWS}
    for _ in range(repeats):
        groups = [(ROWS[:2], None, None), (ROWS[2:5], parent, None), (ROWS[5:], parent, {"MCR_K1_SCREEN": "0", "MCR_K1_SEGMENTS": "0"})]
        for rows, library, env_extra in groups:
            for name, row in run_child(reps, list(rows), library, env_extra).items():
                runs[name].append(row)
    summary = {}
    for name, rows in runs.items():
        medians = [r["median_ms"] for r in rows]
        summary[name] = {"median_ms": statistics.median(medians), "medians_ms": medians, "spread_ms": max(medians) - min(medians),
                         "successes": rows[0]["successes"], **({"row_sums_ok": all(r["row_sums_ok"] for r in rows)} if "row_sums_ok" in rows[0] else {})}
        src = "this build" if name.startswith("rule_bins") or not parent else "parent library"
        print(f"{name:>20} ({src}): median {summary[name]['median_ms']:.3f} ms, medians {[round(m, 3) for m in medians]}, "
              f"spread {summary[name]['spread_ms']:.3f} ms, successes {summary[name]['successes']}"
              + (f", row sums {'ok' if summary[name]['row_sums_ok'] else 'WRONG'}" if "row_sums_ok" in summary[name] else ""), flush=True)
    m = {k: v["median_ms"] for k, v in summary.items()}
    derived = {"plain_bins_increment_ms": m["plain_year_bins"] - m["plain_whole_path"]}
    for rname in RULES:
        a, c = m[f"rule_bins_{rname}"], m[f"rule_count_{rname}"]
        derived[rname] = {"a_over_b": a / m["plain_year_bins"], "a_over_c": a / c, "increment_over_c_ms": a - c}
        print(f"{rname}: (a) / (b) = {a / m['plain_year_bins']:.3f}, (a) / (c) = {a / c:.3f}, (a) - (c) = {a - c:.3f} ms "
              f"against (b) - plain whole path = {derived['plain_bins_increment_ms']:.3f} ms", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump({"n_paths": N_PATHS, "working_months": WM, "bins": [N_BINS] * 3, "reps": reps, "repeats": repeats,
                       "reference_library": "parent" if parent else "this build", "rows": summary, "derived": derived}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
