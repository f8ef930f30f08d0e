"""Income probes: the fan-out route (income fan-out launches, path_kernel PHASE 10) against the per-option route (one
count-only launch per option, forced with MCR_INCOME_FANOUT_MIN_WAVES) and against the same 15 records through the scenario
fan-out (PHASE 8: the same work less the record's stream), on config.json at 240 working months; then the wall time and probe
count of the required-income search.

    python tools/income_probe_timing.py [out.json] [--reps 25] [--quick]

HIP-event medians over --reps calls after warmup, the forms interleaved call by call; prints one line per shape with the
quartiles of the samples and writes every sample to out.json.  Counts of the two income routes are compared for every shape
(bit identity); the scenario fan-out is timed over options that change the three money fields only."""

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

ROUTE = "MCR_INCOME_FANOUT_MIN_WAVES"


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
    money = (cfgd["initial_balance"], cfgd["monthly_contribution"], cfgd["monthly_expenses"])
    # the claim-age ladder of the pension: 60 .. 74, 8 % more for every year of waiting
    options = [money + (round(2800.0 * 1.08 ** k, 2), 60.0 + k, None) for k in range(L)]
    scenarios = [(money[0], money[1], round(money[2] * (0.7 + 0.04 * k), 2)) for k in range(L)]
    rows = []
    for n in shapes:
        def fan():
            os.environ[ROUTE] = "0"
            return E.probe_income(p, seed, 0, 0, n, wm, 0, options)

        def per():
            os.environ[ROUTE] = str(2**40)
            return E.probe_income(p, seed, 0, 0, n, wm, 0, options)

        def scn():
            return E.probe_scenarios(p, seed, 0, 0, n, wm, scenarios)

        for _ in range(3):
            timed(fan), timed(per), timed(scn)
        tf, tp, ts = [], [], []
        same = True
        for _ in range(reps):
            t, a = timed(fan)
            tf.append(t)
            t, b = timed(per)
            tp.append(t)
            t, _ = timed(scn)
            ts.append(t)
            same = same and torch.equal(a, b)
        os.environ.pop(ROUTE, None)
        mf, mp, ms = statistics.median(tf), statistics.median(tp), statistics.median(ts)
        rows.append({"n": n, "options": L, "wm": wm, "fanout_ms": mf, "per_option_ms": mp, "scenario_fanout_ms": ms,
                     "fanout_over_per_option": mf / mp, "fanout_over_scenario_fanout": mf / ms, "identical": same,
                     "fanout_samples": tf, "per_option_samples": tp, "scenario_fanout_samples": ts})
        print(f"n={n:>8} L={L}: income fan-out {mf:8.3f} ms (quartiles {quartiles(tf)[0]:.3f} / {quartiles(tf)[2]:.3f})  "
              f"per-option {mp:8.3f} ms ({quartiles(tp)[0]:.3f} / {quartiles(tp)[2]:.3f})  "
              f"scenario fan-out {ms:8.3f} ms ({quartiles(ts)[0]:.3f} / {quartiles(ts)[2]:.3f})  "
              f"ratios {mf / mp:.3f} {mf / ms:.4f}  identical={same}", flush=True)
    searches = []
    for label, paths in (("find_minimum_income_amount(120, pension from retirement)", cfgd["num_simulations_search"]),
                         ("find_minimum_income_amount(120, pension from retirement) @ 50 000", 50_000)):
        sim = RetirementMonteCarloSimulator(Config(**dict(cfgd, seed=7, num_simulations_search=paths)))
        run = lambda ev: sim.find_minimum_income_amount(120, 0, start_at_age=0.0, verbose=False, progress_callback=ev.append)  # noqa: E731
        run([])   # warm
        times, ev = [], []
        for _ in range(3 if "--quick" in args else 7):
            ev = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = run(ev)
            times.append((time.perf_counter() - t0) * 1e3)
        probes = max(e["iteration"] for e in ev)
        searches.append({"what": label, "search_paths": paths, "wall_ms": times, "median_ms": statistics.median(times),
                         "probe_rounds": probes, "levels_evaluated": len(ev), "answer": res[0]})
        print(f"{label}: median {statistics.median(times):.2f} ms (min {min(times):.2f}, max {max(times):.2f}), {probes} probe rounds, "
              f"{len(ev)} points, answer {res[0]}", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows, "searches": searches}, fh, indent=1)
    return 0 if all(r["identical"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
