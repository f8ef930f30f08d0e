#!/usr/bin/env python3
"""Allocation probes: the eleven splits 0, 0.1, ..., 1 over the same paths, scenarios/config.json at 233 working months (833
months a path), at 50 000 paths (the search's shape) and at 10^6.

    python tools/allocation_probe_timing.py [out.json] [--parent-library PATH/libmcr_hip.so] [--reps 15] [--repeats 3] [--quick]

Rows (HIP-event medians of --reps calls after warm-up -- 20 x --reps calls at the 50 000-path shape, where a call takes a few
milliseconds and 15 of them would be a window of some 30 ms -- each median taken --repeats times in a process of its own: the
spread of those medians is the run-to-run noise):
  fanout        mcr_probe_allocations_rng on the fan-out route (allocation fan-out launches, path_kernel PHASE 12): this build
  per_option    the same entry with MCR_ALLOCATION_FANOUT_MIN_WAVES set huge (one count-only launch per option on side
                streams): this build
  launches      11 count-only launches one after the other, each of a parameter block with its own allocation_inv1_pct: what a
                caller had to issue before the probe existed -- from --parent-library when given (the parent commit's build,
                loaded through MCR_HIP_LIBRARY), else from this build.  THE YARDSTICK.
  search        one find_best_allocation end to end (wall clock, 50 000 search paths, three rounds and the closing joint probe),
                on the fan-out route and with the knob set huge (the same rounds as per-option launches)
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

WM, SEED, STREAM = 233, 12345, 0
SPLITS = [i / 10.0 for i in range(11)]
L = len(SPLITS)
SHAPES = (50_000, 1_000_000)
WARMUP = 3
SMALL_SHAPE, SMALL_SHAPE_REPS = 100_000, 20      # below this many paths a median is taken over SMALL_SHAPE_REPS x --reps calls
KNOB = "MCR_ALLOCATION_FANOUT_MIN_WAVES"


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

    cfgd = json.load(open(os.path.join(REPO, "scenarios", "config.json")))
    row, n = os.environ["ALLOCATION_PROBE_ROW"], int(os.environ["ALLOCATION_PROBE_PATHS"])
    if row == "search":
        sim = RetirementMonteCarloSimulator(Config(**dict(cfgd, seed=7, num_simulations_search=n)))
        res = sim.find_best_allocation(WM, verbose=False)   # warm
        walls, events = [], []
        for _ in range(max(3, reps // 3)):
            events = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = sim.find_best_allocation(WM, verbose=False, progress_callback=events.append)
            walls.append((time.perf_counter() - t0) * 1e3)
        out = {"median_ms": statistics.median(walls), "min_ms": min(walls), "max_ms": max(walls), "answer": res[0], "probability": res[1],
               "tied": res[3], "rounds": max(e["iteration"] for e in events), "points": len(events),
               "fanout_launches_of_the_joint_probe": int(N.load_library().mcr_probe_allocations_last_fanout_launches())}
    else:
        p = params_from_config(Config(**cfgd))
        last = {}
        if row == "launches":
            def launch():
                got = []
                for a in SPLITS:
                    p.allocation_inv1_pct = a
                    got.append(E.probe_months(p, SEED, STREAM, 0, n, [WM]))
                last["counts"] = got
        else:
            records = [(cfgd["initial_balance"], cfgd["monthly_contribution"], cfgd["monthly_expenses"], a) for a in SPLITS]

            def launch():
                last["res"] = E.probe_allocations(p, SEED, STREAM, 0, n, WM, records)
        out = timed(launch, reps)
        if row == "launches":
            flat = torch.cat(last["counts"]).cpu().numpy()
        else:
            flat = last["res"].cpu().numpy()
            out["fanout_launches"] = int(N.load_library().mcr_probe_allocations_last_fanout_launches())
        out["counts"] = flat.tolist()
    print(json.dumps(out), flush=True)
    return 0


def run_child(reps: int, row: str, n: int, library=None, env_extra=None):
    env = dict(os.environ)
    for k in ("MCR_HIP_LIBRARY", KNOB):
        env.pop(k, None)
    if library:
        env["MCR_HIP_LIBRARY"] = library
    env.update(ALLOCATION_PROBE_ROW=row, ALLOCATION_PROBE_PATHS=str(n), **(env_extra or {}))
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
        calls = reps * (SMALL_SHAPE_REPS if n < SMALL_SHAPE else 1)
        for _ in range(repeats):
            runs["fanout"].append(run_child(calls, "fanout", n))
            runs["per_option"].append(run_child(calls, "per_option", n, env_extra={KNOB: str(2 ** 40)}))
            runs["launches"].append(run_child(calls, "launches", n, parent))
        same = all(r["counts"] == runs["launches"][0]["counts"] for rows in runs.values() for r in rows)
        identical = identical and same
        entry = {"n_paths": n, "options": L, "working_months": WM, "calls_per_median": calls, "identical": same, "successes": [c[0] for c in runs["fanout"][0]["counts"]],
                 "fanout_launches": runs["fanout"][0]["fanout_launches"], "per_option_fanout_launches": runs["per_option"][0]["fanout_launches"]}
        for name, rows in runs.items():
            medians = [r["median_ms"] for r in rows]
            entry[name] = {"median_ms": statistics.median(medians), "medians_ms": medians, "spread_ms": max(medians) - min(medians),
                           "library": yardstick if name == "launches" else "this build"}
        entry["fanout_over_launches"] = entry["fanout"]["median_ms"] / entry["launches"]["median_ms"]
        entry["fanout_over_per_option"] = entry["fanout"]["median_ms"] / entry["per_option"]["median_ms"]
        summary.append(entry)
        print(f"n={n:>8} L={L}: " + "  ".join(
            f"{name} ({entry[name]['library']}) {entry[name]['median_ms']:.3f} ms, medians {[round(m, 3) for m in entry[name]['medians_ms']]}"
            for name in runs) + f"  fan-out / launches {entry['fanout_over_launches']:.3f}  fan-out / per-option {entry['fanout_over_per_option']:.3f}"
            f"  identical={same}", flush=True)
    searches = {}
    for name, extra in (("fan-out route", None), ("per-option route", {KNOB: str(2 ** 40)})):
        rows = [run_child(reps * SMALL_SHAPE_REPS, "search", SHAPES[0], env_extra=extra) for _ in range(repeats)]
        medians = [r["median_ms"] for r in rows]
        searches[name] = {"median_ms": statistics.median(medians), "medians_ms": medians, "spread_ms": max(medians) - min(medians),
                          **{k: rows[0][k] for k in ("answer", "probability", "tied", "rounds", "points")}}
        print(f"find_best_allocation({WM}) @ {SHAPES[0]} paths, {name}: median {searches[name]['median_ms']:.2f} ms, medians "
              f"{[round(m, 2) for m in medians]}, {rows[0]['rounds']} rounds, {rows[0]['points']} points, answer {rows[0]['answer']}, "
              f"tied {rows[0]['tied']}", flush=True)
    identical = identical and searches["fan-out route"]["answer"] == searches["per-option route"]["answer"]
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"reps": reps, "repeats": repeats, "yardstick": yardstick, "rows": summary, "searches": searches}, fh, indent=1)
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
