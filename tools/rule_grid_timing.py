#!/usr/bin/env python3
"""Rule-grid probe: retirement months x spending levels under one rule over the same paths, scenarios/config.json at 50 000
paths under the symmetric guardrail, in the two shapes its callers issue:

  search    17 consecutive months x 1 level  (the verification window of find_minimum_working_months_with_rule)
  frontier   6 months x 15 levels            (a round of find_maximum_initial_expenses_by_months)

    python tools/rule_grid_timing.py [out.json] [--parent-library PATH/libmcr_hip.so] [--reps 15] [--repeats 3] [--quick]

Rows (HIP-event medians of --reps calls after warm-up, each median taken --repeats times in a process of its own: the spread
of those medians is the run-to-run noise):
  grid        mcr_probe_rule_grid_rng on the shared route (one sweep, rule grid fan-out launches): this build
  per_row     the same entry with MCR_EXPENSE_FANOUT_MIN_WAVES set huge (mcr_probe_rules_rng per row): this build
  launches    the same cells as individual mcr_run_rule_rng launches one after the other -- from --parent-library when given
              (the parent commit's build, loaded through MCR_HIP_LIBRARY), else from this build.  THE YARDSTICK.
  searches    find_minimum_working_months and find_minimum_working_months_with_rule end to end (wall clock, 50 000 search
              paths) on this build, and the rule search with one rule launch per probed month (what a caller could do before the
              probe existed) on the yardstick's library
Nothing is judged.  The grid's and the per-row route's integers are compared with the launches' (bit identity)."""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SEED, STREAM, N_PATHS = 12345, 0, 50_000
RULE = (1.2, 0.8, 0.10, 0.10, 0.5, 1.5)
SHAPES = {"search": (list(range(217, 234)), 1), "frontier": ([120, 150, 180, 210, 240, 270], 15)}
WARMUP = 3
KNOB = "MCR_EXPENSE_FANOUT_MIN_WAVES"


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
    import torch

    from monte_carlo_retirement_amd import Config, params_from_config
    from monte_carlo_retirement_amd import _native as N
    from monte_carlo_retirement_amd import engine as E
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
    from monte_carlo_retirement_amd.spending_rules import SpendingRule

    cfgd = json.load(open(os.path.join(REPO, "scenarios", "config.json")))
    row, shape = os.environ["RULE_GRID_ROW"], os.environ["RULE_GRID_SHAPE"]
    rule = N.McrSpendingRule(*RULE)
    if row.startswith("search_"):
        sim = RetirementMonteCarloSimulator(Config(**dict(cfgd, seed=7, num_simulations_search=N_PATHS)))
        srule = SpendingRule(*RULE)
        if row == "search_rule_launches":     # one rule launch per probed month: no probe is needed
            def per_month(months, n, rule_):
                return {int(m): sim._count_percent(sim._rule_counts(int(m), rule_, sim._current_params(), int(n))[0], int(n)) for m in months}

            sim._probe_many_with_rule = per_month
        run = sim.find_minimum_working_months if row == "search_fixed" else (lambda **k: sim.find_minimum_working_months_with_rule(srule, **k))
        res = run(verbose=False)              # warm
        walls = []
        for _ in range(max(3, reps // 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = run(verbose=False)
            walls.append((time.perf_counter() - t0) * 1e3)
        out = {"median_ms": statistics.median(walls), "min_ms": min(walls), "max_ms": max(walls), "months": res[0], "probability": res[1],
               "probes": len(res[2])}
    else:
        months, n_levels = SHAPES[shape]
        base = float(cfgd["monthly_expenses"])
        rows = [[base] if n_levels == 1 else [round(base * (0.4 + 0.1 * k), 2) for k in range(n_levels)] for _ in months]
        p = params_from_config(Config(**cfgd))
        last = {}
        if row == "launches":
            def launch():
                got = []
                for wm, levels in zip(months, rows):
                    for x in levels:
                        p.monthly_expenses = x
                        got.append(E.run_rule(p, SEED, STREAM, 0, N_PATHS, wm, rule)["counts"])
                last["counts"] = got
        else:
            def launch():
                last["res"] = E.probe_rule_grid(p, SEED, STREAM, 0, N_PATHS, months, rows, rule)
        out = timed(launch, reps)
        if row == "launches":
            flat = torch.stack(last["counts"]).cpu().numpy()
        else:
            cells = len(months) * n_levels
            flat = torch.cat([last["res"][0].reshape(cells, -1), last["res"][1].reshape(cells, -1)], dim=1).cpu().numpy()
            out["fanout_launches"] = int(N.load_library().mcr_probe_rule_grid_last_fanout_launches())
        out["counts"] = np.asarray(flat).tolist()
    print(json.dumps(out), flush=True)
    return 0


def run_child(reps: int, row: str, shape: str, library=None, env_extra=None):
    env = dict(os.environ)
    for k in ("MCR_HIP_LIBRARY", KNOB):
        env.pop(k, None)
    if library:
        env["MCR_HIP_LIBRARY"] = library
    env.update(RULE_GRID_ROW=row, RULE_GRID_SHAPE=shape, **(env_extra or {}))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({row}, {shape}, {library or 'this build'}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def spread(rows):
    medians = [r["median_ms"] for r in rows]
    return {"median_ms": statistics.median(medians), "medians_ms": medians, "spread_ms": max(medians) - min(medians)}


def main() -> int:
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 15
    if "--child" in args:
        return child(reps)
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 3
    if "--quick" in args:
        reps, repeats = 5, 1
    parent = os.path.abspath(args[args.index("--parent-library") + 1]) if "--parent-library" in args else None
    out_path = next((a for a in args if a.endswith(".json")), None)
    yardstick = "parent library" if parent else "this build"
    summary, identical = [], True
    for shape, (months, n_levels) in SHAPES.items():
        runs = {"grid": [], "per_row": [], "launches": []}
        for _ in range(repeats):
            runs["grid"].append(run_child(reps, "grid", shape))
            runs["per_row"].append(run_child(reps, "per_row", shape, env_extra={KNOB: str(2 ** 40)}))
            runs["launches"].append(run_child(reps, "launches", shape, parent))
        same = all(r["counts"] == runs["launches"][0]["counts"] for rows in runs.values() for r in rows)
        identical = identical and same
        entry = {"shape": shape, "n_paths": N_PATHS, "months": len(months), "levels": n_levels, "identical": same,
                 "fanout_launches": runs["grid"][0]["fanout_launches"], "per_row_fanout_launches": runs["per_row"][0]["fanout_launches"]}
        for name, rows in runs.items():
            entry[name] = dict(spread(rows), library=yardstick if name == "launches" else "this build")
        entry["grid_over_launches"] = entry["grid"]["median_ms"] / entry["launches"]["median_ms"]
        summary.append(entry)
        print(f"{shape:>8} {len(months)} x {n_levels} @ {N_PATHS}: " + "  ".join(
            f"{name} ({entry[name]['library']}) {entry[name]['median_ms']:.3f} ms, medians {[round(m, 3) for m in entry[name]['medians_ms']]}"
            for name in runs) + f"  grid / launches {entry['grid_over_launches']:.3f}  identical={same}", flush=True)
    searches = {}
    for name, row, library in (("find_minimum_working_months", "search_fixed", None),
                               ("find_minimum_working_months_with_rule", "search_rule", None),
                               (f"rule search, one launch per month ({yardstick})", "search_rule_launches", parent)):
        rows = [run_child(reps, row, "search", library) for _ in range(repeats)]
        searches[name] = dict(spread(rows), **{k: rows[0][k] for k in ("months", "probability", "probes")})
        print(f"{name} @ {N_PATHS} paths: median {searches[name]['median_ms']:.2f} ms, medians "
              f"{[round(m, 2) for m in searches[name]['medians_ms']]}, {rows[0]['probes']} months reported, answer {rows[0]['months']}", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"reps": reps, "repeats": repeats, "yardstick": yardstick, "rows": summary, "searches": searches}, fh, indent=1)
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
