"""Scenario probes: the fan-out route (scenario fan-out launches, path_kernel PHASE 8) against the per-scenario route (one
count-only launch per scenario, forced with MCR_SCENARIO_FANOUT_MIN_WAVES) and against the same 15 levels through the
contribution fan-out (PHASE 7: the same work less three scalar reads), on config.json at 240 working months; then the wall
time and probe count of the required-starting-balance search and of a 5-level withdrawal-rate curve.

    python tools/scenario_probe_timing.py [out.json] [--reps 25] [--quick]

HIP-event medians over --reps calls after warmup, the three forms interleaved call by call; prints one line per shape with
the quartiles of the samples and writes every sample to out.json.  Counts of the three forms are compared for every shape
(bit identity)."""

from __future__ import annotations

import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator  # noqa: E402

ROUTE = "MCR_SCENARIO_FANOUT_MIN_WAVES"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return q[0], q[1], q[2]


def main() -> int:
    args = sys.argv[1:]
    out_path = next((a for a in args if a.endswith(".json")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 25
    shapes = [50_000, 1_000_000]
    if "--quick" in args:
        reps = 5
    cfgd = load_config_from_json(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenarios", "config.json"))
    p = params_from_config(Config(**cfgd))
    wm, seed, L = 240, 12345, 15
    levels = [round(cfgd["monthly_contribution"] * (0.4 + 0.1 * k), 2) for k in range(L)]
    records = [(cfgd["initial_balance"], x, cfgd["monthly_expenses"]) for x in levels]
    rows = []
    for n in shapes:
        def fan():
            os.environ[ROUTE] = "0"
            return E.probe_scenarios(p, seed, 0, 0, n, wm, records)

        def per():
            os.environ[ROUTE] = str(2**40)
            return E.probe_scenarios(p, seed, 0, 0, n, wm, records)

        def con():
            return E.probe_contributions(p, seed, 0, 0, n, wm, levels)

        for _ in range(3):
            timed(fan), timed(per), timed(con)
        tf, tp, tc = [], [], []
        same = True
        for _ in range(reps):
            t, a = timed(fan)
            tf.append(t)
            t, b = timed(per)
            tp.append(t)
            t, c = timed(con)
            tc.append(t)
            same = same and torch.equal(a, b) and torch.equal(a, c)
        os.environ.pop(ROUTE, None)
        mf, mp, mc = statistics.median(tf), statistics.median(tp), statistics.median(tc)
        rows.append({"n": n, "scenarios": L, "wm": wm, "fanout_ms": mf, "per_scenario_ms": mp, "contribution_fanout_ms": mc,
                     "fanout_over_per_scenario": mf / mp, "fanout_over_contribution_fanout": mf / mc, "identical": same,
                     "fanout_samples": tf, "per_scenario_samples": tp, "contribution_fanout_samples": tc})
        print(f"n={n:>8} L={L}: scenario fan-out {mf:8.3f} ms (quartiles {quartiles(tf)[0]:.3f} / {quartiles(tf)[2]:.3f})  "
              f"per-scenario {mp:8.3f} ms ({quartiles(tp)[0]:.3f} / {quartiles(tp)[2]:.3f})  "
              f"contribution fan-out {mc:8.3f} ms ({quartiles(tc)[0]:.3f} / {quartiles(tc)[2]:.3f})  "
              f"ratios {mf / mp:.3f} {mf / mc:.4f}  identical={same}", flush=True)
    searches = []
    for label, paths, fn in (
        ("find_minimum_initial_balance(0)", cfgd["num_simulations_search"], lambda s, ev: s.find_minimum_initial_balance(0, verbose=False, progress_callback=ev.append)),
        ("find_minimum_initial_balance(0) @ 50 000", 50_000, lambda s, ev: s.find_minimum_initial_balance(0, verbose=False, progress_callback=ev.append)),
        ("by_expenses(0, 5 levels) @ 50 000", 50_000, lambda s, ev: s.find_minimum_initial_balance_by_expenses(
            0, [4000.0, 6000.0, 8000.0, 10000.0, 12000.0], verbose=False, progress_callback=ev.append)),
    ):
        sim = RetirementMonteCarloSimulator(Config(**dict(cfgd, seed=7, num_simulations_search=paths)))
        fn(sim, [])   # warm
        times, ev = [], []
        for _ in range(3 if "--quick" in args else 7):
            ev = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(sim, ev)
            times.append((time.perf_counter() - t0) * 1e3)
        probes = max(e["iteration"] for e in ev)
        answer = res[0] if isinstance(res, tuple) else [r[0] for r in res]
        searches.append({"what": label, "search_paths": paths, "wall_ms": times, "median_ms": statistics.median(times),
                         "probe_rounds": probes, "levels_evaluated": len(ev), "answer": answer})
        print(f"{label}: median {statistics.median(times):.2f} ms (min {min(times):.2f}, max {max(times):.2f}), {probes} probe rounds, "
              f"{len(ev)} points, answer {answer}", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows, "searches": searches}, fh, indent=1)
    return 0 if all(r["identical"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
