#!/usr/bin/env python3
"""Rule probes: 15 spending levels under one rule over the same paths, scenarios/config.json at 233 working months (833 months a
path), at 50 000 paths (the search's shape) and at 10^6.

    python tools/rule_probe_timing.py [out.json] [--parent-library PATH/libmcr_hip.so] [--reps 15] [--repeats 3] [--quick]

Rows (HIP-event medians of --reps calls after warm-up, each median taken --repeats times in a process of its own: the spread
of those medians is the run-to-run noise):
  fanout        mcr_probe_rules_rng on the fan-out route (rule fan-out launches, path_kernel PHASE 11): this build
  per_option    the same entry with MCR_RULE_FANOUT_MIN_WAVES set huge (one rule launch per option on side streams): this build
  launches      15 mcr_run_rule_rng launches one after the other, what success_probability_with_rule issued per round before
                the probe existed -- from --parent-library when given (the parent commit's build, loaded through
                MCR_HIP_LIBRARY), else from this build.  THE YARDSTICK.
  search        one find_maximum_initial_expenses end to end (wall clock, 50 000 search paths), on this build and on the parent
                library (whose rounds are one launch per level, as the parent commit's method ran them)
Nothing is judged.  The fan-out's and the per-option route's counts are compared with the launches' (bit identity)."""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WM, SEED, STREAM, L = 233, 12345, 0, 15
RULE = (1.2, 0.8, 0.10, 0.10, 0.5, 1.5)
SHAPES = (50_000, 1_000_000)
WARMUP = 3
KNOB = "MCR_RULE_FANOUT_MIN_WAVES"


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
    import torch

    from monte_carlo_retirement_amd import Config, params_from_config
    from monte_carlo_retirement_amd import _native as N
    from monte_carlo_retirement_amd import engine as E
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator
    from monte_carlo_retirement_amd.spending_rules import SpendingRule

    cfgd = json.load(open(os.path.join(REPO, "scenarios", "config.json")))
    row, n = os.environ["RULE_PROBE_ROW"], int(os.environ["RULE_PROBE_PATHS"])
    rule = N.McrSpendingRule(*RULE)
    levels = [round(cfgd["monthly_expenses"] * (0.4 + 0.1 * k), 2) for k in range(L)]
    has_probe = hasattr(N.load_library(), "mcr_probe_rules_rng")
    out = {}
    if row == "search":
        sim = RetirementMonteCarloSimulator(Config(**dict(cfgd, seed=7, num_simulations_search=n)))
        if not has_probe:     # the parent commit's rounds: one launch per level
            def per_level(working_months, records, count):
                import numpy as np

                rows = []
                for r in records:
                    q = params_from_config(sim.params_model)
                    q.initial_balance, q.monthly_contribution, q.monthly_expenses = r[:3]
                    rows.append(sim._rule_counts(working_months, r[3], q, count))
                return np.array(rows)

            sim._rule_probe_counts = per_level
        srule = SpendingRule(*RULE)
        res = sim.find_maximum_initial_expenses(WM, srule, verbose=False)   # warm
        walls, events = [], []
        for _ in range(max(3, reps // 3)):
            events = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = sim.find_maximum_initial_expenses(WM, srule, verbose=False, progress_callback=events.append)
            walls.append((time.perf_counter() - t0) * 1e3)
        out = {"median_ms": statistics.median(walls), "min_ms": min(walls), "max_ms": max(walls), "answer": res[0], "probability": res[1],
               "rounds": max(e["iteration"] for e in events), "levels": len(events), "probe": has_probe}
    else:
        p = params_from_config(Config(**cfgd))
        last = {}
        if row == "launches":
            def launch():
                got = []
                for x in levels:
                    p.monthly_expenses = x
                    got.append(E.run_rule(p, SEED, STREAM, 0, n, WM, rule)["counts"])
                last["counts"] = got
        else:
            records = [(cfgd["initial_balance"], cfgd["monthly_contribution"], x, rule) for x in levels]

            def launch():
                last["res"] = E.probe_rules(p, SEED, STREAM, 0, n, WM, records)
        out = timed(launch, reps)
        if row == "launches":
            flat = torch.stack(last["counts"]).cpu().numpy()
        else:
            flat = torch.cat([last["res"][0], last["res"][1].reshape(L, -1)], dim=1).cpu().numpy()
            out["fanout_launches"] = int(N.load_library().mcr_probe_rules_last_fanout_launches())
        out["counts"] = flat.tolist()
    print(json.dumps(out), flush=True)
    return 0


def run_child(reps: int, row: str, n: int, library=None, env_extra=None):
    env = dict(os.environ)
    for k in ("MCR_HIP_LIBRARY", KNOB):
        env.pop(k, None)
    if library:
        env["MCR_HIP_LIBRARY"] = library
    env.update(RULE_PROBE_ROW=row, RULE_PROBE_PATHS=str(n), **(env_extra or {}))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({row}, {n} paths, {library or 'this build'}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


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
    for n in SHAPES:
        runs = {"fanout": [], "per_option": [], "launches": []}
        for _ in range(repeats):
            runs["fanout"].append(run_child(reps, "fanout", n))
            runs["per_option"].append(run_child(reps, "per_option", n, env_extra={KNOB: str(2 ** 40)}))
            runs["launches"].append(run_child(reps, "launches", n, parent))
        same = all(r["counts"] == runs["launches"][0]["counts"] for rows in runs.values() for r in rows)
        identical = identical and same
        entry = {"n_paths": n, "options": L, "working_months": WM, "identical": same,
                 "fanout_launches": runs["fanout"][0]["fanout_launches"], "per_option_fanout_launches": runs["per_option"][0]["fanout_launches"]}
        for name, rows in runs.items():
            medians = [r["median_ms"] for r in rows]
            entry[name] = {"median_ms": statistics.median(medians), "medians_ms": medians, "spread_ms": max(medians) - min(medians),
                           "library": yardstick if name == "launches" else "this build"}
        entry["fanout_over_launches"] = entry["fanout"]["median_ms"] / entry["launches"]["median_ms"]
        summary.append(entry)
        print(f"n={n:>8} L={L}: " + "  ".join(
            f"{name} ({entry[name]['library']}) {entry[name]['median_ms']:.3f} ms, medians {[round(m, 3) for m in entry[name]['medians_ms']]}"
            for name in runs) + f"  fan-out / launches {entry['fanout_over_launches']:.3f}  identical={same}", flush=True)
    searches = {}
    for name, library in (("this build", None), ("parent library", parent)):
        if name == "parent library" and not parent:
            continue
        rows = [run_child(reps, "search", SHAPES[0], library) for _ in range(repeats)]
        medians = [r["median_ms"] for r in rows]
        searches[name] = {"median_ms": statistics.median(medians), "medians_ms": medians, "spread_ms": max(medians) - min(medians),
                          **{k: rows[0][k] for k in ("answer", "probability", "rounds", "levels", "probe")}}
        print(f"find_maximum_initial_expenses({WM}) @ {SHAPES[0]} paths, {name}: median {searches[name]['median_ms']:.2f} ms, medians "
              f"{[round(m, 2) for m in medians]}, {rows[0]['rounds']} rounds, {rows[0]['levels']} levels, answer {rows[0]['answer']}", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"reps": reps, "repeats": repeats, "yardstick": yardstick, "rows": summary, "searches": searches}, fh, indent=1)
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
