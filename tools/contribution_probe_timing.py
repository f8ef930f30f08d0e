"""Contribution probes: the fan-out route (contribution fan-out launches, path_kernel PHASE 7) against the per-level route
(one count-only launch per level, forced with MCR_CONTRIBUTION_FANOUT_MIN_WAVES), on config.json at 240 working months.

    python tools/contribution_probe_timing.py [out.json] [--reps 25] [--quick]

HIP-event medians over --reps calls after warmup, the two routes interleaved call by call; prints one line per shape and
writes every sample to out.json.  Counts of both routes are compared for every shape (bit identity)."""

from __future__ import annotations

import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402

ROUTE = "MCR_CONTRIBUTION_FANOUT_MIN_WAVES"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main() -> int:
    args = sys.argv[1:]
    out_path = next((a for a in args if a.endswith(".json")), None)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 25
    shapes = [(n, L) for n in (50_000, 1_000_000) for L in (2, 4, 8, 15)]
    if "--quick" in args:
        shapes, reps = [(50_000, 8), (1_000_000, 8)], 5
    cfgd = load_config_from_json(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenarios", "config.json"))
    p = params_from_config(Config(**cfgd))
    wm, seed = 240, 12345
    rows = []
    for n, L in shapes:
        levels = [round(cfgd["monthly_contribution"] * (0.4 + 0.1 * k), 2) for k in range(L)]

        def fan():
            os.environ[ROUTE] = "0"
            return E.probe_contributions(p, seed, 0, 0, n, wm, levels)

        def per():
            os.environ[ROUTE] = str(2**40)
            return E.probe_contributions(p, seed, 0, 0, n, wm, levels)

        for _ in range(3):
            timed(fan), timed(per)
        tf, tp = [], []
        same = True
        for _ in range(reps):
            t, a = timed(fan)
            tf.append(t)
            t, b = timed(per)
            tp.append(t)
            same = same and torch.equal(a, b)
        os.environ.pop(ROUTE, None)
        mf, mp = statistics.median(tf), statistics.median(tp)
        row = {"n": n, "levels": L, "wm": wm, "fanout_ms": mf, "per_level_ms": mp, "ratio": mf / mp, "identical": same,
               "fanout_samples": tf, "per_level_samples": tp}
        rows.append(row)
        print(f"n={n:>8} L={L:>2}: fan-out {mf:8.3f} ms  per-level {mp:8.3f} ms  ratio {mf / mp:.3f}  identical={same}", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows}, fh, indent=1)
    return 0 if all(r["identical"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
