#!/usr/bin/env python3
"""Glide probes against the allocation probe: eleven options over the same paths, scenarios/config.json at 233 working months
(833 months a path), at 50 000 paths and at 10^6.  What it shows is the cost of the yearly reload of a consumer wave's weight.

    python tools/glide_probe_timing.py [out.json] [--parent-library PATH/libmcr_hip.so] [--reps 15] [--repeats 3] [--quick]

Rows (HIP-event medians of --reps calls after warm-up -- 20 x --reps calls at the 50 000-path shape, where a call takes a few
milliseconds -- each median taken --repeats times in a process of its own: the spread of those medians is the run-to-run noise):
  glide              mcr_probe_glide_paths_rng (path_kernel PHASE 13), eleven tables that change in every year of the horizon
  glide_constant     the same entry, eleven tables of one entry: the splits 0, 0.1, ..., 1 (no reload ever loads)
  allocation         mcr_probe_allocations_rng (PHASE 12) of the same eleven constant splits: this build.  THE COMPARISON.
  allocation_parent  the same call on --parent-library (the parent commit's build, loaded through MCR_HIP_LIBRARY), where
                     given: the regression guard for the allocation probe, whose kernels the ISA fingerprint shows unchanged
Nothing is judged.  The counts of glide_constant are compared with the allocation rows' (bit identity)."""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WM, SEED, STREAM = 233, 12345, 0
SPLITS = [i / 10.0 for i in range(11)]
L = len(SPLITS)
SHAPES = (50_000, 1_000_000)
WARMUP = 3
SMALL_SHAPE, SMALL_SHAPE_REPS = 100_000, 20      # below this many paths a median is taken over SMALL_SHAPE_REPS x --reps calls


def yearly_tables(years: int):
    """Eleven tables whose every entry differs from the one before it."""
    return [tuple(round(0.05 + 0.9 * (((7 * y + 3 * k) % 19) / 18.0), 6) for y in range(years)) for k in range(L)]


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

    cfgd = json.load(open(os.path.join(REPO, "scenarios", "config.json")))
    row, n = os.environ["GLIDE_PROBE_ROW"], int(os.environ["GLIDE_PROBE_PATHS"])
    p = params_from_config(Config(**cfgd))
    amounts = (cfgd["initial_balance"], cfgd["monthly_contribution"], cfgd["monthly_expenses"])
    last = {}
    if row.startswith("allocation"):
        records = [amounts + (a,) for a in SPLITS]

        def launch():
            last["res"] = E.probe_allocations(p, SEED, STREAM, 0, n, WM, records)
        counter = "mcr_probe_allocations_last_fanout_launches"
    else:
        years = (WM + 12 * int(cfgd["retirement_years"]) + 11) // 12
        tables = [(a,) for a in SPLITS] if row == "glide_constant" else yearly_tables(years)
        records = [amounts + (t,) for t in tables]

        def launch():
            last["res"] = E.probe_glide_paths(p, SEED, STREAM, 0, n, WM, records)
        counter = "mcr_probe_glide_paths_last_fanout_launches"
    out = timed(launch, reps)
    out["counts"] = last["res"].cpu().numpy().tolist()
    out["fanout_launches"] = int(getattr(N.load_library(), counter)())
    print(json.dumps(out), flush=True)
    return 0


def run_child(reps: int, row: str, n: int, library=None):
    env = dict(os.environ)
    for k in ("MCR_HIP_LIBRARY", "MCR_ALLOCATION_FANOUT_MIN_WAVES", "MCR_GLIDE_FANOUT_MIN_WAVES"):
        env.pop(k, None)
    if library:
        env["MCR_HIP_LIBRARY"] = library
    env.update(GLIDE_PROBE_ROW=row, GLIDE_PROBE_PATHS=str(n))
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
    names = ["glide", "glide_constant", "allocation"] + (["allocation_parent"] if parent else [])
    summary, identical = [], True
    for n in SHAPES:
        runs = {name: [] for name in names}
        calls = reps * (SMALL_SHAPE_REPS if n < SMALL_SHAPE else 1)
        for _ in range(repeats):
            for name in names:
                runs[name].append(run_child(calls, name, n, parent if name == "allocation_parent" else None))
        same = all(r["counts"] == runs["allocation"][0]["counts"] for name in names if name != "glide" for r in runs[name])
        identical = identical and same
        entry = {"n_paths": n, "options": L, "working_months": WM, "calls_per_median": calls, "constant_tables_identical": same,
                 "successes": {name: [c[0] for c in runs[name][0]["counts"]] for name in ("glide", "allocation")},
                 "fanout_launches": {name: runs[name][0]["fanout_launches"] for name in names}}
        for name, rows in runs.items():
            medians = [r["median_ms"] for r in rows]
            entry[name] = {"median_ms": statistics.median(medians), "medians_ms": medians, "spread_ms": max(medians) - min(medians)}
        entry["glide_over_allocation"] = entry["glide"]["median_ms"] / entry["allocation"]["median_ms"]
        summary.append(entry)
        print(f"n={n:>8} L={L}: " + "  ".join(f"{name} {entry[name]['median_ms']:.3f} ms, medians {[round(m, 3) for m in entry[name]['medians_ms']]}"
                                               for name in names) + f"  glide / allocation {entry['glide_over_allocation']:.4f}  identical={same}", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"reps": reps, "repeats": repeats, "parent_library": bool(parent), "rows": summary}, fh, indent=1)
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
