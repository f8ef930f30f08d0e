"""Assumption probes: the default stress table (15 records) at 240 working months through
  baseline    a loop of engine.probe_months(params_k, ..., [wm]), one parameter block per record — what the table cost before
              mcr_probe_assumptions_rng existed; on the library named by --baseline-library (a libmcr_hip.so built from the
              parent commit) when given, else on this tree's (its plain launches are the parent's instruction streams),
  fan-out     mcr_probe_assumptions_rng with MCR_ASSUMPTION_FANOUT_MIN_WAVES=0 (path_kernel PHASE 9),
  per-record  the same call with MCR_ASSUMPTION_FANOUT_MIN_WAVES=2^40 (one count-only launch per record on the side streams),
on config.json and jorge.json at 50 000 and 10^6 paths.

    python tools/assumption_probe_timing.py [out.json] [--reps 25] [--quick] [--baseline-library PATH [--baseline-label TEXT]]

HIP-event times over --reps calls after warmup, the three forms interleaved call by call; prints the median and the quartiles per
shape, says whether the fan-out's inter-quartile range lies wholly below the baseline's (the rule for the default of
MCR_ASSUMPTION_FANOUT_MIN_WAVES, LABNOTES R13), and writes every sample to out.json.  The counts of the three forms are
compared for every shape (bit identity).  out.json names the baseline's library by --baseline-label when given (a description
such as the commit it was built from, where the path would mean nothing to a reader), else by its path."""

from __future__ import annotations

import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config  # noqa: E402
from monte_carlo_retirement_amd import _native as N  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402
from monte_carlo_retirement_amd.stress import assumption_records, stress_scenarios  # noqa: E402

ROUTE = "MCR_ASSUMPTION_FANOUT_MIN_WAVES"


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
    if "--quick" in args:
        reps = 5
    this_lib = N.load_library()
    base_lib = this_lib
    base_path = args[args.index("--baseline-library") + 1] if "--baseline-library" in args else None
    base_label = args[args.index("--baseline-label") + 1] if "--baseline-label" in args else base_path
    if base_path:
        base_lib = C.CDLL(base_path)
        N._declare(base_lib)
    wm, seed = 240, 12345
    rows = []
    for name in ("config.json", "jorge.json"):
        cfgd = load_config_from_json(os.path.join(REPO, "scenarios", name))
        cfg = Config(**cfgd)
        p = params_from_config(cfg)
        table = stress_scenarios(cfg)
        records = assumption_records(cfg, [o for _, o in table])
        blocks = [params_from_config(Config(**dict(cfgd, **o))) for _, o in table]
        for n in (50_000, 1_000_000):
            def baseline():
                N._lib = base_lib
                try:
                    return torch.cat([E.probe_months(q, seed, 0, 0, n, [wm]) for q in blocks])
                finally:
                    N._lib = this_lib

            def fan():
                os.environ[ROUTE] = "0"
                return E.probe_assumptions(p, seed, 0, 0, n, wm, records)

            def per():
                os.environ[ROUTE] = str(2**40)
                return E.probe_assumptions(p, seed, 0, 0, n, wm, records)

            for _ in range(3):
                timed(baseline), timed(fan), timed(per)
            tb, tf, tp = [], [], []
            same = True
            for _ in range(reps):
                t, a = timed(baseline)
                tb.append(t)
                t, b = timed(fan)
                tf.append(t)
                t, c = timed(per)
                tp.append(t)
                same = same and torch.equal(a, b) and torch.equal(a, c)
            os.environ.pop(ROUTE, None)
            qb, qf, qp = quartiles(tb), quartiles(tf), quartiles(tp)
            below = qf[2] < qb[0]
            rows.append({"config": name, "n": n, "records": len(records), "wm": wm, "baseline_ms": qb[1], "fanout_ms": qf[1],
                         "per_record_ms": qp[1], "baseline_quartiles": [qb[0], qb[2]], "fanout_quartiles": [qf[0], qf[2]],
                         "per_record_quartiles": [qp[0], qp[2]], "fanout_over_baseline": qf[1] / qb[1],
                         "fanout_iqr_below_baseline_iqr": below, "identical": same,
                         "baseline_samples": tb, "fanout_samples": tf, "per_record_samples": tp})
            print(f"{name:>11} n={n:>8} L={len(records)}: baseline {qb[1]:8.3f} ms (quartiles {qb[0]:.3f} / {qb[2]:.3f})  "
                  f"fan-out {qf[1]:8.3f} ms ({qf[0]:.3f} / {qf[2]:.3f})  per-record {qp[1]:8.3f} ms ({qp[0]:.3f} / {qp[2]:.3f})  "
                  f"fan-out / baseline {qf[1] / qb[1]:.3f}  IQR below baseline's: {below}  identical={same}", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "baseline_library": base_label or "this tree's",
                       "rows": rows}, fh, indent=1)
    return 0 if all(r["identical"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
