"""Soak of the screened count-only route ("Screened count-only launches"): the screening kernel alone
(mcr_screen_paths_rng) against the fp64 path kernel with per-path outputs, over K1_SOAK_PATHS paths (default 2 000 000) of
four plans.  Must show ZERO paths classed SAFE that the fp64 kernel fails.  Prints per plan: the doubtful share, the lowest
cap / need among SAFE paths and the largest |final_total / final_balance - 1| over them.

    python tools/screen_soak.py [first_path]
"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
n = int(os.environ.get("K1_SOAK_PATHS", "2000000"))
begin = int(sys.argv[1]) if len(sys.argv) > 1 else 0


def scenario(name="config.json", **over):
    return dict(json.load(open(os.path.join(root, "scenarios", name))), **over)


PLANS = [("config.json wm233", scenario(), 233),
         ("S60 wm120", scenario(initial_balance=2.0e6, inv1_returns_volatility=0.15, equity_inflation_correlation=0.3), 120),
         ("jorge.json rho 0.3 wm75", scenario("jorge.json", equity_inflation_correlation=0.3), 75),
         ("config.json expenses 40000 wm233", scenario(monthly_expenses=40000.0), 233)]
bad_total = 0
for name, cfgd, wm in PLANS:
    p = params_from_config(Config(**cfgd))
    s = E.screen_paths(p, 12345, 1, begin, n, wm)
    r = E.run_batch_host(p, 12345, 1, begin, n, wm, want_trajectories=False)
    safe = s["cls"] == 0
    bad = int((safe & ((r["success"] == 0) | ~np.isnan(r["years_to_ruin"]))).sum())
    bad_total += bad
    dev = np.abs(s["final_total"][safe].astype(np.float64) / r["final_balance"][safe] - 1.0) if safe.any() else np.zeros(1)
    low = float(s["min_ratio"][safe].min()) if safe.any() else float("inf")
    print(f"{name:34s} paths {begin}..{begin + n}: doubtful {1.0 - safe.mean():.5f}  fp64 failures {int((r['success'] == 0).sum()):8d}  "
          f"SAFE that fail in fp64 {bad}  lowest min_ratio among SAFE {low:.3f}  max |final_total / final_balance - 1| {dev.max():.3e}", flush=True)
print("soak:", "ok, no SAFE path fails" if bad_total == 0 else f"FAILED, {bad_total} SAFE paths fail")
sys.exit(0 if bad_total == 0 else 1)
