#!/usr/bin/env python3
"""The glide whole-path launches against the routes the tree had before them: ONE glide path over scenarios/config.json at 233
working months (833 months a path), at 50 000 paths and at 10^6.

    python tools/glide_run_timing.py [out.json] [--parent-library PATH/libmcr_hip.so] [--reps 15] [--repeats 3] [--quick]

Rows (HIP-event medians of --reps calls after warm-up -- 20 x --reps calls at the 50 000-path shape, where a call takes a fraction
of a millisecond -- each median taken --repeats times in a process of its own: the spread of those medians is the run-to-run
noise).  Every call writes into buffers allocated before the first one.
  glide_count          mcr_run_glide_rng, count-only (path_kernel MODE 0, GLIDE), a table that changes in every year of the horizon
  glide_count_one      the same entry, a table of one entry: the plan's own split (no reload ever loads)
  probe_parent         (a) the same single option through mcr_probe_glide_paths_rng on --parent-library (the parent commit's build,
                       loaded through MCR_HIP_LIBRARY): the only route that build has, a 128-thread fan-out workgroup of one
                       producer and one consumer wave.  Same table as glide_count; the success count must be the same.
  probe_parent_one     ... under the one-entry table
  plain_count          (b) this build's plain count-only mcr_run_batch_rng as it routes itself (the screened / growth / month /
                       stream forms the host picks for the plan): the product's answer for a constant split
  plain_count_generic  the same launch held to the forms the glide kernels have (MCR_K1_SCREEN=0, growth, month and stream form 0):
                       glide_count_one against this row is the cost of the month counter and the reload; against plain_count, of
                       not having the launch-constant forms as well
  glide_bins           mcr_run_glide_year_bins_rng (MODE 3, GLIDE), 256 + 256 bins, the yearly table
  glide_bins_one       ... the one-entry table
  plain_bins           (c) mcr_run_year_bins_rng on the same edges
Nothing is judged.  What is compared: the success count of glide_count with probe_parent's, the integers of glide_count_one with
plain_count's and plain_count_generic's, the whole vector of glide_bins_one with plain_bins'."""
from __future__ import annotations

import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WM, SEED, STREAM = 233, 12345, 0
SHAPES = (50_000, 1_000_000)
WARMUP = 3
SMALL_SHAPE, SMALL_SHAPE_REPS = 100_000, 20      # below this many paths a median is taken over SMALL_SHAPE_REPS x --reps calls
GENERIC_FORMS = {"MCR_K1_SCREEN": "0", "MCR_K1_GROWTH_FORM": "0", "MCR_K1_MONTH_FORM": "0", "MCR_K1_STREAM_FORM": "0"}
ROWS = ("glide_count", "glide_count_one", "probe_parent", "probe_parent_one", "plain_count", "plain_count_generic",
        "glide_bins", "glide_bins_one", "plain_bins")


def yearly_table(years: int):
    """A table whose every entry differs from the one before it."""
    return tuple(round(0.05 + 0.9 * (((7 * y + 3) % 19) / 18.0), 6) for y in range(years))


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

    cfgd = json.load(open(os.path.join(REPO, "scenarios", "config.json")))
    row, n = os.environ["GLIDE_RUN_ROW"], int(os.environ["GLIDE_RUN_PATHS"])
    p = params_from_config(Config(**cfgd))
    lib = N.load_library()
    rng = N.philox_rng(SEED)
    sz = E.query_sizes(p, WM)
    ry = int(sz.retirement_years)
    years = (WM + 12 * ry + 11) // 12
    weights = (float(cfgd["allocation_inv1_pct"]),) if row.endswith("_one") else yearly_table(years)
    table = (C.c_double * len(weights))(*weights)
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    out = {}
    if row.endswith("_bins") or "_bins_" in row:
        batch = E.YearBinsBatch(p, WM, glide_path=None if row == "plain_bins" else weights)

        def launch():
            batch.launch(SEED, STREAM, 0, n)

        def answer():       # (the launches accumulate: one launch into a zeroed vector)
            batch.zero()
            launch()
            return batch.reduce_vec.cpu().numpy().tolist()
    elif row.startswith("probe_parent"):
        counts = torch.zeros(N.MCR_N_COUNTERS, dtype=torch.int64, device="cuda")
        option = (N.McrGlideOption * 1)(N.McrGlideOption(float(cfgd["initial_balance"]), float(cfgd["monthly_contribution"]),
                                                           float(cfgd["monthly_expenses"]), 0, len(weights)))

        def launch():
            N.check(lib.mcr_probe_glide_paths_rng(C.byref(p), C.byref(rng), STREAM, 0, n, WM, table, len(weights), option, 1,
                                                  C.c_void_p(counts.data_ptr()), 0, stream), "mcr_probe_glide_paths_rng")

        def answer():       # (the probe zeroes its counters in every call)
            return counts.cpu().numpy().tolist()
    else:
        ints = torch.zeros(N.MCR_N_COUNTERS + ry + int(sz.ruin_bins), dtype=torch.int64, device="cuda")
        o = N.McrOutputs()
        o.path_stride = n
        o.counters, o.wr_obs_counts, o.ruin_year_bins = ints.data_ptr(), ints[N.MCR_N_COUNTERS:].data_ptr(), ints[N.MCR_N_COUNTERS + ry:].data_ptr()
        if row.startswith("glide_count"):
            def launch():
                N.check(lib.mcr_run_glide_rng(C.byref(p), C.byref(rng), STREAM, 0, n, WM, table, len(weights), C.byref(o), 0, stream), "mcr_run_glide_rng")
        else:
            def launch():
                N.check(lib.mcr_run_batch_rng(C.byref(p), C.byref(rng), STREAM, 0, n, WM, None, C.byref(o), 0, stream), "mcr_run_batch_rng")

        def answer():       # (the launches accumulate: one launch into zeroed integers)
            ints.zero_()
            launch()
            return ints.cpu().numpy().tolist()
    out = timed(launch, reps)
    out["answer"] = answer()
    print(json.dumps(out), flush=True)
    return 0


def run_child(reps: int, row: str, n: int, library=None):
    env = dict(os.environ)
    for k in ("MCR_HIP_LIBRARY", "MCR_GLIDE_FANOUT_MIN_WAVES", *GENERIC_FORMS):
        env.pop(k, None)
    if library:
        env["MCR_HIP_LIBRARY"] = library
    if row == "plain_count_generic":
        env.update(GENERIC_FORMS)
    env.update(GLIDE_RUN_ROW=row, GLIDE_RUN_PATHS=str(n))
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
    names = [r for r in ROWS if parent or not r.startswith("probe_parent")]
    summary, identical = [], True
    for n in SHAPES:
        runs = {name: [] for name in names}
        calls = reps * (SMALL_SHAPE_REPS if n < SMALL_SHAPE else 1)
        for _ in range(repeats):
            for name in names:
                runs[name].append(run_child(calls, name, n, parent if name.startswith("probe_parent") else None))
        ans = {name: runs[name][0]["answer"] for name in names}
        same = {"glide_count_one == plain_count": ans["glide_count_one"] == ans["plain_count"] == ans["plain_count_generic"],
                "glide_bins_one == plain_bins": ans["glide_bins_one"] == ans["plain_bins"],
                "every repeat gives the same answer": all(r["answer"] == ans[name] for name in names for r in runs[name])}
        if parent:
            same["glide_count == probe_parent"] = ans["glide_count"][:2] == ans["probe_parent"][:2] and ans["glide_count_one"][:2] == ans["probe_parent_one"][:2]
        identical = identical and all(same.values())
        entry = {"n_paths": n, "working_months": WM, "calls_per_median": calls, "answers_identical": same,
                 "successes": {name: ans[name][0] for name in names}}
        for name, rows in runs.items():
            medians = [r["median_ms"] for r in rows]
            entry[name] = {"median_ms": statistics.median(medians), "medians_ms": medians, "spread_ms": max(medians) - min(medians)}
        ratio = lambda a, b: entry[a]["median_ms"] / entry[b]["median_ms"]      # noqa: E731
        entry["ratios"] = {"(b) glide_count_one / plain_count": ratio("glide_count_one", "plain_count"),
                           "(b) glide_count_one / plain_count_generic": ratio("glide_count_one", "plain_count_generic"),
                           "(c) glide_bins_one / plain_bins": ratio("glide_bins_one", "plain_bins"),
                           "glide_bins / plain_bins": ratio("glide_bins", "plain_bins")}
        if parent:
            entry["ratios"]["(a) glide_count / probe_parent"] = ratio("glide_count", "probe_parent")
            entry["ratios"]["(a) glide_count_one / probe_parent_one"] = ratio("glide_count_one", "probe_parent_one")
        summary.append(entry)
        print(f"n={n:>8}: " + "  ".join(f"{name} {entry[name]['median_ms']:.4f} ms {[round(m, 4) for m in entry[name]['medians_ms']]}" for name in names), flush=True)
        print(f"           ratios {({k: round(v, 4) for k, v in entry['ratios'].items()})}  identical={same}", flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump({"reps": reps, "repeats": repeats, "parent_library": bool(parent), "rows": summary}, fh, indent=1)
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
