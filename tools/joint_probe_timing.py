"""Joint probes: what `mcr_probe_income_joint_rng` costs over `mcr_probe_income_rng`, on the shapes of income_probe_timing.py
(config.json, 15 claim-age options, 240 working months, 50 000 and 10^6 paths).

    python tools/joint_probe_timing.py [out.json] [--reps 25] [--quick] [--parent-library PATH]

In one process, interleaved call by call, HIP-event times after warmup: the plain probe; the joint probe with caller-owned
masks and with the library's scratch masks; `mcr_joint_counts` alone on the masks the joint probe left; and at 50 000 paths
the per-option route (MCR_INCOME_FANOUT_MIN_WAVES huge) of the plain and of the joint probe.  The expectation to confirm or
refute: joint = plain + the reduction, within the run-to-run spread of the plain probe.  Checks that the joint call's counts
equal the plain probe's and that both routes give the same masks and matrix.

--parent-library: a libmcr_hip.so built from the parent commit.  The plain probe is then also timed in fresh processes that
load this tree's library and the parent's in turn (new, parent, parent, new: a library is chosen when a process loads it), which
gives the parent's own run-to-run spread and whether the plain probe moved."""

from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402

ROUTE = "MCR_INCOME_FANOUT_MIN_WAVES"
WM, SEED, L = 240, 12345, 15
SHAPES = [50_000, 1_000_000]


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


def plan():
    cfgd = load_config_from_json(os.path.join(REPO, "scenarios", "config.json"))
    money = (cfgd["initial_balance"], cfgd["monthly_contribution"], cfgd["monthly_expenses"])
    # the claim-age ladder of the pension: 60 .. 74, 8 % more for every year of waiting
    return params_from_config(Config(**cfgd)), [money + (round(2800.0 * 1.08 ** k, 2), 60.0 + k, None) for k in range(L)]


def interleave(forms, reps, warm=3):
    """forms: name -> callable.  Returns name -> samples (ms), the forms called in turn."""
    for _ in range(warm):
        for fn in forms.values():
            timed(fn)
    samples = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            samples[k].append(timed(fn)[0])
    return samples


def child(reps):
    """The plain probe alone, in this process's library: one JSON line."""
    p, options = plan()
    os.environ[ROUTE] = "0"
    out = {}
    for n in SHAPES:
        s = interleave({"plain": lambda: E.probe_income(p, SEED, 0, 0, n, WM, 0, options)}, reps)["plain"]
        out[str(n)] = {"median_ms": statistics.median(s), "samples": s,
                       "counts": E.probe_income(p, SEED, 0, 0, n, WM, 0, options).cpu().numpy().tolist()}
    print(json.dumps(out), flush=True)
    return 0


def across_processes(parent_library, reps):
    rows = []
    for label in ("new", "parent", "parent", "new"):
        env = dict(os.environ)
        env.pop("MCR_HIP_LIBRARY", None)
        if label == "parent":
            env["MCR_HIP_LIBRARY"] = parent_library
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"{label} child failed: {r.stderr[-2000:]}")
        rows.append({"library": label, **json.loads(r.stdout.strip().splitlines()[-1])})
        print(f"process {len(rows)} ({label:>6}): plain probe " +
              "  ".join(f"n={n}: {rows[-1][str(n)]['median_ms']:.3f} ms" for n in SHAPES), flush=True)
    same = all(r[str(n)]["counts"] == rows[0][str(n)]["counts"] for r in rows for n in SHAPES)
    summary = {}
    for n in SHAPES:
        med = {lab: [r[str(n)]["median_ms"] for r in rows if r["library"] == lab] for lab in ("new", "parent")}
        summary[str(n)] = {"new_medians_ms": med["new"], "parent_medians_ms": med["parent"],
                           "parent_spread_ms": max(med["parent"]) - min(med["parent"]), "new_spread_ms": max(med["new"]) - min(med["new"]),
                           "new_minus_parent_ms": statistics.mean(med["new"]) - statistics.mean(med["parent"])}
        print(f"n={n}: parent {med['parent']}, new {med['new']} ms; new - parent = {summary[str(n)]['new_minus_parent_ms']:+.4f} ms", flush=True)
    return {"processes": rows, "summary": summary, "counts_identical": same}


def main() -> int:
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 25
    if "--quick" in args:
        reps = 5
    if "--child" in args:
        return child(reps)
    out_path = next((a for a in args if a.endswith(".json")), None)
    doc = {"reps": reps, "options": L, "wm": WM}
    ok = True
    if "--parent-library" in args:   # (first: this process has not opened the GPU yet)
        doc["plain_probe_across_processes"] = across_processes(os.path.abspath(args[args.index("--parent-library") + 1]), reps)
        ok = doc["plain_probe_across_processes"]["counts_identical"]
    p, options = plan()
    rows = []
    for n in SHAPES:
        os.environ[ROUTE] = "0"
        counts, joint, extremes, masks = E.probe_income_joint(p, SEED, 0, 0, n, WM, 0, options)
        plain_counts = E.probe_income(p, SEED, 0, 0, n, WM, 0, options)
        same = torch.equal(counts, plain_counts) and torch.equal(joint.diagonal(), counts[:, 0])

        def route(waves, fn):
            def call():
                os.environ[ROUTE] = waves
                return fn()
            return call

        forms = {
            "plain": route("0", lambda: E.probe_income(p, SEED, 0, 0, n, WM, 0, options)),
            "joint": route("0", lambda: E.probe_income_joint(p, SEED, 0, 0, n, WM, 0, options)),
            "joint_scratch_masks": route("0", lambda: E.probe_income_joint(p, SEED, 0, 0, n, WM, 0, options, masks=None)),
            "reduction": lambda: E.joint_counts(masks, n),
        }
        if n <= 50_000:
            forms["plain_per_option"] = route(str(2**40), lambda: E.probe_income(p, SEED, 0, 0, n, WM, 0, options))
            forms["joint_per_option"] = route(str(2**40), lambda: E.probe_income_joint(p, SEED, 0, 0, n, WM, 0, options))
            os.environ[ROUTE] = str(2**40)
            c2, j2, e2, m2 = E.probe_income_joint(p, SEED, 0, 0, n, WM, 0, options)
            same = same and torch.equal(c2, counts) and torch.equal(j2, joint) and torch.equal(e2, extremes) and torch.equal(m2, masks)
        samples = interleave(forms, reps)
        os.environ.pop(ROUTE, None)
        med = {k: statistics.median(v) for k, v in samples.items()}
        q = quartiles(samples["plain"])
        row = {"n": n, "identical": bool(same), "median_ms": med, "plain_interquartile_ms": q[2] - q[0],
               "joint_minus_plain_ms": med["joint"] - med["plain"],
               "joint_minus_plain_minus_reduction_ms": med["joint"] - med["plain"] - med["reduction"],
               "mask_bytes": int(masks.numel() * 8), "all_succeed": int(extremes[0]), "none_succeed": int(extremes[1]), "samples": samples}
        rows.append(row)
        ok = ok and bool(same)
        print(f"n={n:>8} L={L}: " + "  ".join(f"{k} {v:.3f}" for k, v in med.items()) +
              f" ms; plain IQR {q[2] - q[0]:.3f}; joint - plain = {row['joint_minus_plain_ms']:+.3f}, less the reduction "
              f"{row['joint_minus_plain_minus_reduction_ms']:+.3f}; identical={same}", flush=True)
    doc.update(device=torch.cuda.get_device_name(0), rows=rows)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(doc, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
