"""The plans tests/count_fuzz.py generates are worth running: mixed outcomes, few dropped for their money scale, every class
filled, and every compiled count-only variant of the path kernel (tax masks 0-3, growth masks 0 / 1 / 3, month form 1, the
pre-retirement failures of the annual-gains kernels, the last rate below the exact-month switch) reached by some plan.  The
generator, the CPU oracle and the host's form choice (mcr_k1_growth_form / mcr_k1_month_form) only: no device needed.

The same for the plans' NumPy leg (rng="numpy", shocks drawn by NumPy and injected into the oracle): below the money scale,
mixed, every variant family of that stream reached, the seed recipe equal to the long-hand one; and the comparison functions
of tests/test_gpu_numpy_stream_vs_oracle.py reject a stream that is wrong in one of three ways."""

from __future__ import annotations

import time

import pytest

import count_fuzz as F
from monte_carlo_retirement_amd import engine as E

KNOBS = ("MCR_K1_GROWTH_FORM", "MCR_K1_MONTH_FORM")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _tax_mask(cfgd) -> int:
    """derive_params: an asset carries an effective realized-gains rate when it uses that system at a rate above 0."""
    return sum(bit for bit, a in ((1, "inv1"), (2, "inv2")) if cfgd[f"{a}_use_realized_gains_tax_system"] and cfgd[f"{a}_realized_gains_tax_rate"] > 0)


def _annual(cfgd) -> bool:
    return any(not cfgd[f"{a}_use_realized_gains_tax_system"] and cfgd[f"{a}_annual_tax_on_gains_rate"] > 0 for a in ("inv1", "inv2"))


def test_the_generated_plans_meet_their_conditions(oracle):
    t0 = time.time()
    plans = {cls: F.scenarios(oracle, cls) for cls in F.CLASSES}
    seconds = time.time() - t0
    kept = [s for cls in F.CLASSES for s in plans[cls]]
    shares = {(s.cls, s.index): F.failure_share(F.oracle_run(oracle, s, trajectories=True)) for s in kept}
    mixed = [k for k, v in shares.items() if F.MIXED[0] <= v <= F.MIXED[1]]
    growth = {m: 0 for m in (0, 1, 3)}
    month = {m: 0 for m in (0, 1)}
    tax = {m: 0 for m in range(4)}
    pre_retirement = below_exact = 0
    for s in kept:
        p = s.params()
        growth[E.growth_form(p, s.wm)] += 1
        month[E.month_form(p, s.wm)] += 1
        tax[_tax_mask(s.cfgd)] += 1
        run = F.oracle_run(oracle, s, trajectories=True)
        assert F.money_scale(run) < F.SCALE_LIMIT, s.context()
        assert int(run["counters"][1]) == s.n == F.PATHS[s.index % 2]
        pre_retirement += int(run["ruin_year_bins"][0])
        below_exact += any(s.cfgd[f"{a}_use_realized_gains_tax_system"] and s.cfgd[f"{a}_realized_gains_tax_rate"] == F.RATE_BELOW_EXACT
                           for a in ("inv1", "inv2"))
    drawn = sum(F.STATS[cls]["drawn"] for cls in F.CLASSES)
    dropped = sum(F.STATS[cls]["dropped_scale"] for cls in F.CLASSES)
    print(f"count_fuzz seed {F.seed()}: {len(kept)} kept of {drawn} drawn in {seconds:.1f} s, {dropped} dropped for a money scale >= 2^33, "
          f"{len(mixed)} mixed; growth masks {growth}, month forms {month}, tax masks {tax}, "
          f"pre-retirement failures {pre_retirement}, plans at rate 1 - 2e-6: {below_exact}")
    for cls in F.CLASSES:
        print(f"  {cls}: {F.STATS[cls]}")
        assert len(plans[cls]) == F.KEPT[cls] >= 8, cls
    assert len(mixed) >= 0.9 * len(kept), sorted((k, round(v, 3)) for k, v in shares.items() if k not in mixed)
    assert dropped <= 0.05 * drawn, (dropped, drawn)
    assert min(growth.values()) >= 8, growth
    assert month[1] >= 8, month
    assert min(tax.values()) >= 1, tax
    assert pre_retirement > 0
    assert below_exact >= 1
    # every class is what its name says
    for s in kept:
        p, mask, annual = s.params(), _tax_mask(s.cfgd), _annual(s.cfgd)
        paying = sum(1 for x in s.cfgd["other_income_streams"] if x["monthly_amount_today"] != 0.0)
        exact = any(s.cfgd[f"{a}_use_realized_gains_tax_system"] and s.cfgd[f"{a}_realized_gains_tax_rate"] > 1.0 - 1e-6 for a in ("inv1", "inv2"))
        assert len(E.kept_streams(p, s.wm)) == paying
        if s.cls == "generic":
            assert (paying > 16) != exact and not annual, s.context()
            continue
        assert paying <= 6 and not exact, s.context()
        assert annual == (s.cls == "annual"), s.context()
        if s.cls != "annual":
            assert mask == {"equal_rates": 3, "unequal_rates": 3, "mask1": 1, "mask2": 2, "mask0": 0}[s.cls], s.context()
            assert E.month_form(p, s.wm) == (1 if s.cls == "equal_rates" else 0), s.context()


def test_the_plans_do_not_depend_on_the_order_of_generation(oracle):
    """A class's plans are a function of the seed and the class alone (the GPU tests generate class by class)."""
    again, _ = F._generate(oracle, "mask2", 3)
    assert [(s.cfgd, s.wm, s.seed, s.stream, s.begin, s.n) for s in again] == \
           [(s.cfgd, s.wm, s.seed, s.stream, s.begin, s.n) for s in F.scenarios(oracle, "mask2")[:3]]


# ---- the NumPy leg of the plans (count_fuzz.numpy_leg ...): tests/test_gpu_numpy_stream_vs_oracle.py runs them on the device ----
FAMILIES = ("tax form 3, no annual tax", "tax form 0, no annual tax", "tax form 0, annual tax", "tax form 3, annual tax",
            "generic, tolerance month", "generic, exact month")


def _paying(cfgd) -> int:
    return sum(1 for x in cfgd["other_income_streams"] if x["monthly_amount_today"] != 0.0)


def _exact(cfgd) -> bool:
    return any(cfgd[f"{a}_use_realized_gains_tax_system"] and cfgd[f"{a}_realized_gains_tax_rate"] > 1.0 - 1e-6 for a in ("inv1", "inv2"))


def _numpy_family(cfgd) -> str:
    """The path_kernel<MODE, 1, ...> family a plan runs on the NumPy stream (for_whole_path_variant in csrc/mcr_hip.hip): the
    generic form for more than 16 paying streams or the exact month; else taxed (mask 3, a zero rate as exact zeros) or untaxed,
    with or without the annual-gains tax."""
    if _exact(cfgd):
        return "generic, exact month"
    if _paying(cfgd) > 16:
        return "generic, tolerance month"
    return f"tax form {3 if _tax_mask(cfgd) else 0}, {'annual' if _annual(cfgd) else 'no annual'} tax"


def test_the_plans_are_worth_running_on_the_numpy_stream(oracle):
    import numpy as np

    t0 = time.time()
    plans = [s for cls in F.CLASSES for s in F.scenarios(oracle, cls)]
    t1 = time.time()
    extra = F.numpy_extra(oracle)
    runs = {(s.cls, s.index): F.oracle_run_numpy(oracle, s, trajectories=True) for s in plans + extra}
    seconds = time.time() - t1
    families = {f: 0 for f in FAMILIES}
    one_sided = {1: 0, 2: 0}
    mixed, below_exact, pre_retirement, legs = [], 0, 0, set()
    for s in plans + extra:
        run = runs[s.cls, s.index]
        # a plan over the scale fails the test: nothing is dropped here (the classes' plans were chosen on the Philox stream)
        assert F.money_scale(run) < F.SCALE_LIMIT, (F.money_scale(run), s.context("NumPy stream"))
        assert int(run["counters"][1]) == s.n == F.PATHS[s.index % 2]
        families[_numpy_family(s.cfgd)] += 1
        if _tax_mask(s.cfgd) in one_sided and not _exact(s.cfgd) and _paying(s.cfgd) <= 16:
            one_sided[_tax_mask(s.cfgd)] += 1           # runs as mask 3 "with exact zeros"
        if F.MIXED[0] <= F.failure_share(run) <= F.MIXED[1]:
            mixed.append((s.cls, s.index))
        below_exact += any(s.cfgd[f"{a}_use_realized_gains_tax_system"] and s.cfgd[f"{a}_realized_gains_tax_rate"] == F.RATE_BELOW_EXACT
                           for a in ("inv1", "inv2"))
        pre_retirement += int(run["ruin_year_bins"][0]) > 0
        legs.add(F.numpy_leg(s)[1:])
    print(f"NumPy leg, count_fuzz seed {F.seed()}: {len(plans)} class plans + {len(extra)} extra ({F.STATS[F.EXTRA]}); drawing and injecting "
          f"took {seconds:.1f} s (the class plans' generation {t1 - t0:.1f} s, 0.0 if another test made them); 0 over the 2^33 money "
          f"scale, {len(mixed)} of {len(plans) + len(extra)} mixed; one-sided masks run as mask 3: {one_sided}; plans at rate "
          f"1 - 2e-6: {below_exact}; plans with pre-retirement failures: {pre_retirement}; (child_offset, path_begin) legs: {sorted(legs)}")
    for f in FAMILIES:
        print(f"  {f}: {families[f]}")
    assert len(mixed) >= 0.9 * (len(plans) + len(extra)), sorted(set(runs) - set(mixed))
    assert min(families.values()) >= 4, families
    assert min(one_sided.values()) >= 1, one_sided
    assert below_exact >= 1 and pre_retirement >= 1
    assert any(off > 0 for off, _ in legs) and any(begin > 0 for _, begin in legs), legs
    # the supplement is the family the classes leave out: the generic variant WITH an annual-gains tax
    assert len(extra) == F.EXTRA_KEPT
    for s in extra:
        assert _numpy_family(s.cfgd) == "generic, tolerance month" and _annual(s.cfgd) and _paying(s.cfgd) > 16, s.context()
        assert len(E.kept_streams(s.params(), s.wm)) == _paying(s.cfgd)
    assert not any(_annual(s.cfgd) for s in plans if s.cls == "generic")
    # the recipe, the long way: SeedSequence(main).spawn(2)[stream].spawn(..)[child], one word of state, default_rng, the rho mix
    for s in (F.scenarios(oracle, "equal_rates")[0], F.scenarios(oracle, "mask0")[1], F.scenarios(oracle, "annual")[5], extra[1]):
        main, off, begin = F.numpy_leg(s)
        rows = oracle.query_sizes(s.params(), s.wm).shock_rows
        children = np.random.SeedSequence(main).spawn(2)[s.stream].spawn(off + begin + s.n)
        rho = s.cfgd["equity_inflation_correlation"]
        got = F.numpy_shocks(s)
        assert got.shape == (s.n, rows, 3) and got.dtype == np.float64
        for i in range(s.n):
            seed32 = int(children[off + begin + i].generate_state(1)[0])
            ind = np.random.default_rng(seed32).standard_normal((rows, 3))
            exp = np.column_stack((ind[:, 0], rho * ind[:, 0] + np.sqrt(max(0.0, 1.0 - rho * rho)) * ind[:, 1], ind[:, 2]))
            assert np.array_equal(got[i].view(np.uint64), exp.view(np.uint64)), (i, s.context("numpy_shocks"))
    assert {F.numpy_leg(s)[1:] for s in (F.scenarios(oracle, "mask0")[1], F.scenarios(oracle, "annual")[5])} == {(7, 0), (100_000, 1000)}


def _as_launches(run):
    """What the four launches of tests/test_gpu_numpy_stream_vs_oracle.py would return for a kernel that computes `run`."""
    import numpy as np

    from test_gpu_numpy_stream_vs_oracle import EDGES, _cells

    ok = run["success"].astype(bool)
    ints = {k: run[k] for k in ("counters", "ruin_year_bins", "wr_obs_counts")}
    edges, wr_edges = E.default_year_edges(), E.default_wr_edges()
    bins = lambda data, e: np.stack([_cells(r[~np.isnan(r)], e) for r in data])     # noqa: E731
    count = dict(ints, hist_bins=np.histogram(run["final_balance"][ok], bins=EDGES)[0])
    year = dict(ints, edges=edges, wr_edges=wr_edges, trajectory_bins=bins(run["trajectory"], edges),
                real_trajectory_bins=bins(run["real_trajectory"], edges), wr_bins=bins(run["withdrawal_rate_trajectory"], wr_edges),
                final_success_bins=_cells(run["final_balance"][ok], edges))
    return {"full": run, "summary": run, "count": count, "year": year}


def test_the_numpy_stream_comparisons_reject_a_wrong_stream(oracle):
    """The comparison functions of tests/test_gpu_numpy_stream_vs_oracle.py can fail: a "kernel" that consumes the shock rows one
    late, takes the premium's column for the inflation's, or forgets the rho mix is rejected by each of them, on at least one
    plan of every class.  (The oracle stands in for the kernel: no device.)"""
    import numpy as np

    import test_gpu_numpy_stream_vs_oracle as T

    checks = {"full": T.same_full_output, "summary": T.same_summary, "count": T.same_count_only, "year": T.same_year_bins}
    t0 = time.time()
    rejected = {}
    for cls in F.CLASSES + (F.EXTRA,):
        plans = [s for s in F.numpy_plans(oracle, cls) if s.cfgd["equity_inflation_correlation"] != 0.0][:3]
        assert plans, cls
        for s in plans:
            ora = F.oracle_run_numpy(oracle, s, trajectories=True)
            for name, check in checks.items():          # the unperturbed run passes every comparison
                check(s, _as_launches(ora)[name], ora)
            shocks = F.numpy_shocks(s)
            wrong = {"rows shifted by one": np.concatenate([shocks[:, 1:], shocks[:, -1:]], axis=1),
                     "columns 1 and 2 swapped": shocks[:, :, [0, 2, 1]],
                     "rho = 0": F.numpy_shocks(s, rho=0.0)}
            for what, bad in wrong.items():
                run = oracle.run_batch(s.params(), 0, s.stream, 0, s.n, s.wm, injected_shocks=bad, want_trajectories=True)
                launches = _as_launches(run)
                for name, check in checks.items():
                    try:
                        check(s, launches[name], ora)
                    except AssertionError:
                        rejected[cls, what, name] = rejected.get((cls, what, name), 0) + 1
    print(f"catch check ({time.time() - t0:.1f} s): plans rejected, of the first three with rho != 0 of each class")
    for cls in F.CLASSES + (F.EXTRA,):
        for what in ("rows shifted by one", "columns 1 and 2 swapped", "rho = 0"):
            row = {name: rejected.get((cls, what, name), 0) for name in checks}
            print(f"  {cls}: {what}: {row}")
            assert min(row.values()) >= 1, (cls, what, row)
