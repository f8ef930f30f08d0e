"""Stratified random plans for the count-only routes of the path kernel, with the CPU oracle's answer to each.

tests/test_gpu_differential.py draws its plans from one distribution, which never yields a block that qualifies for the
equal-rates month form and almost never one inside the narrow exp window.  Here every plan is drawn for a named CLASS, so that
each compiled count-only variant (tax masks 0-3, the annual-gains kernels, the generic extended-stream / exact-month ones) gets
parameter blocks of its own, and the growth-form ingredients (rho, the volatilities) are strata of the plan's index within its
class rather than left to chance:

    index % 5 in (0, 4): rho = 0          index % 5 in (1, 3): rho uniform in (-1, 1)          index % 5 == 2: rho = +-1
    index % 4 == 1:      equity volatility 0.2-0.6 (outside the narrow exp window: growth mask 0)

A count on a plan where every path succeeds (or fails) proves little, so `monthly_expenses` is calibrated after the draw, with
the oracle alone: ten bisection steps on log-expenses in [20, 200 000] at 128 paths towards half the paths failing.  A plan that
is still all-or-nothing at the test's path count (no wealth at all, income that covers everything) is drawn again, at most
MAX_ATTEMPTS times.  A plan one of whose paths reaches a money scale (max |trajectory|) of 2^33 is DROPPED and counted: from
there on the reference's absolute 1e-6 comparisons are below one ulp of their operands and its own flags hang on the last bit
of exp (tests/test_gpu_differential.py), so only below it are identical counts demanded.

Every plan also has a NumPy leg (`numpy_leg`, `numpy_shocks`, `oracle_run_numpy` at the end of the file): the same plan on the
reference's own random stream, its shocks drawn by NumPy and injected into the oracle, for the rng="numpy" kernels; and
`numpy_extra` adds the one variant family of that stream the classes leave out.  The classes' plans do not depend on it.

The SCREENED family (`screened_scenarios`, at the end of the file) is drawn for the one count-only route the classes' plans do
not reach, the fp32 screening kernel and its fp64 re-run; it has generators of its own, and no other plan depends on it.

MCR_COUNT_FUZZ_SEED: other plans (soaks by hand); the default is the suite's.  Everything is deterministic in it, class by
class: a class's plans do not depend on which other classes were generated before."""

from __future__ import annotations

import math
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

from monte_carlo_retirement_amd import Config, params_from_config

CLASSES = ("equal_rates", "unequal_rates", "mask1", "mask2", "mask0", "annual", "generic")
KEPT = {"equal_rates": 10, "unequal_rates": 10, "mask1": 10, "mask2": 10, "mask0": 10, "annual": 10, "generic": 8}
SLICED_CLASSES = ("equal_rates", "mask1", "annual")
PATHS = (512, 321)                      # even / odd index: two whole workgroups; a ragged last wavefront and workgroup
SCALE_LIMIT = 2.0 ** 33
RATE_BELOW_EXACT = 1.0 - 2e-6           # the last rate class below the exact-month switch (rate > 1 - 1e-6)
MAX_ATTEMPTS = 8
CAL_PATHS, CAL_STEPS, CAL_LO, CAL_HI = 128, 10, 20.0, 200_000.0
MIXED = (0.05, 0.95)
SAMPLE = 4096                           # trajectory sample of a time-sliced plan (its money scale, its failure share)


def seed() -> int:
    return int(os.environ.get("MCR_COUNT_FUZZ_SEED", "20261018"))


@dataclass
class Scenario:
    cls: str
    index: int
    cfgd: dict
    wm: int
    seed: int
    stream: int
    begin: int
    n: int

    def config(self, **over) -> Config:
        return Config(**dict(self.cfgd, **over))

    def params(self, **over):
        return params_from_config(self.config(**over))

    def frozen_streams(self) -> int:
        """Paying non-indexed income streams: the lock columns the kernel keeps."""
        return sum(1 for s in self.cfgd["other_income_streams"] if not s["inflation_indexed"] and s["monthly_amount_today"] != 0.0)

    def context(self, route: str = "", env=None) -> str:
        return (f"class {self.cls} scenario {self.index} route {route!r} env {dict(env or {})}: seed={self.seed} stream={self.stream} "
                f"path_begin={self.begin} n={self.n} wm={self.wm} cfg={self.cfgd}")


# ---- the draw ---------------------------------------------------------------------------------------------------------------
def _streams(rng, pick, age, count):
    out = []
    for s in range(count):
        out.append({
            "name": f"s{s}", "monthly_amount_today": float(pick(0.0, rng.uniform(50, 4000), rng.uniform(50, 4000))),
            "start_at_age": float(age + rng.uniform(-3, 25)), "duration_years": pick(None, int(rng.integers(0, 12))),
            "inflation_indexed": bool(rng.integers(2)), "tax_rate": float(pick(0.0, 1.0, rng.uniform(0, 0.6))),
        })
    return out


def _tax(cls, rng, pick, i):
    """The twelve tax fields' six values of class `cls`: (use1, real1, annual1, use2, real2, annual2)."""
    rate = lambda: float(pick(rng.uniform(0.01, 0.6), rng.uniform(0.01, 0.6), 0.1, RATE_BELOW_EXACT))  # noqa: E731
    ignored = lambda: float(pick(0.0, rng.uniform(0, 0.5)))    # noqa: E731  (an annual rate on an asset of the realized system is not applied)
    untaxed = lambda: pick((False, float(pick(0.0, rng.uniform(0, 0.6))), 0.0), (True, 0.0, ignored()))  # noqa: E731  annual system at rate 0 | realized at rate 0
    if cls == "equal_rates":
        r = float((rng.uniform(0.01, 0.6), 0.1, RATE_BELOW_EXACT)[i % 3])
        return (True, r, ignored(), True, r, ignored())
    if cls == "unequal_rates":
        r1, r2 = rate(), rate()
        while r2 == r1:
            r2 = float(rng.uniform(0.01, 0.6))
        return (True, r1, ignored(), True, r2, ignored())
    if cls == "mask1":
        return (True, rate(), ignored()) + untaxed()
    if cls == "mask2":
        return untaxed() + (True, rate(), ignored())
    if cls == "mask0":
        return untaxed() + untaxed()
    if cls == "annual":
        annual = lambda: (False, float(pick(0.0, rng.uniform(0, 0.6))), float(pick(1.0, rng.uniform(0.05, 0.5), rng.uniform(0.05, 0.5))))  # noqa: E731
        other = lambda: pick((True, rate(), ignored()), untaxed())  # noqa: E731
        return (annual() + other(), other() + annual(), annual() + annual())[i % 3]
    raise ValueError(cls)


def _draw(cls, rng, i, n):
    pick = lambda *xs: xs[int(rng.integers(len(xs)))]  # noqa: E731
    age = float(pick(25.0, 40.5, 58.25, 66.0))
    wm = int(pick(0, 1, 11, 12, 13, 25, int(rng.integers(0, 200))))
    outside = i % 4 == 1
    rho = (0.0, float(rng.uniform(-1, 1)), float(pick(-1.0, 1.0)), float(rng.uniform(-1, 1)), 0.0)[i % 5]
    n_streams = int(rng.integers(0, 7))
    base = cls
    if cls == "generic":   # even: 17-20 paying streams on a lean class's taxes; odd: a realized rate the exact month is for
        base = pick("equal_rates", "unequal_rates", "mask1", "mask2", "mask0") if i % 2 == 0 else pick("equal_rates", "mask1", "mask2")
    use1, real1, ann1, use2, real2, ann2 = _tax(base, rng, pick, i)
    if cls == "generic" and i % 2 == 1:
        exact = float(pick(1.0, 1.0 - 5e-7))     # mask1 / mask2: on the taxed asset; else on asset 1, and on both for i % 4 == 1
        if base != "mask2":
            real1 = exact
        if base == "mask2" or (base == "equal_rates" and i % 4 == 1):
            real2 = exact
    streams = _streams(rng, pick, age, n_streams)
    if cls == "generic" and i % 2 == 0:
        streams = _streams(rng, pick, age, int(rng.integers(20, 26)))
        for s in streams[:int(rng.integers(17, 21))]:       # at least 17 of them pay: one beyond the by-value block of 16
            s["monthly_amount_today"] = float(rng.uniform(20, 400))
    cfgd = dict(
        scenario=f"{cls}-{i}", initial_balance=float(pick(0.0, rng.uniform(1e3, 5e4), rng.uniform(1e5, 1e6))),
        monthly_contribution=float(pick(0.0, rng.uniform(0, 5000), rng.uniform(0, 5000))),
        contribution_growth_rate_annual=float(rng.uniform(0, 0.06)) if i % 2 else 0.0,
        monthly_expenses=1000.0, current_age=age, retirement_years=int(rng.integers(4, 41)),
        allocation_inv1_pct=float(pick(0.0, 1.0, rng.uniform(0, 1), rng.uniform(0, 1))),
        inv1_returns_mean=float(rng.uniform(-0.02, 0.12)),
        inv1_returns_volatility=float(rng.uniform(0.2, 0.6)) if outside else float(pick(0.0, rng.uniform(0.02, 0.17), rng.uniform(0.02, 0.17))),
        inv1_annual_tax_on_gains_rate=ann1, inv1_realized_gains_tax_rate=real1, inv1_use_realized_gains_tax_system=use1,
        inv2_premium_over_inflation_mean=float(rng.uniform(-0.02, 0.05)),
        inv2_premium_over_inflation_volatility=float(pick(0.0, rng.uniform(0, 0.12), rng.uniform(0, 0.12))),
        inv2_annual_tax_on_gains_rate=ann2, inv2_realized_gains_tax_rate=real2, inv2_use_realized_gains_tax_system=use2,
        inflation_rate_mean=float(rng.uniform(-0.01, 0.08)), inflation_rate_volatility=float(pick(0.0, rng.uniform(0, 0.04), rng.uniform(0, 0.04))),
        equity_inflation_correlation=rho,
        num_simulations_main=1, num_simulations_search=1, target_probability=50.0, starting_working_months_search=0,
        seed=None, num_processes=1, other_income_streams=streams,
    )
    if cls == "annual" and i % 5 == 4:
        # the family of test_gpu_differential.py prone to PRE-RETIREMENT annual-tax failure: inv1 booms and is taxed annually at
        # 100 %, its gains are swept into inv2, which crashes
        cfgd.update(allocation_inv1_pct=0.5, inv1_returns_mean=1.5, inv1_returns_volatility=0.5,
                    inv1_use_realized_gains_tax_system=False, inv1_annual_tax_on_gains_rate=1.0,
                    inv2_premium_over_inflation_mean=-0.9, inv2_premium_over_inflation_volatility=0.3,
                    inv2_use_realized_gains_tax_system=True, inv2_realized_gains_tax_rate=0.5,
                    inflation_rate_mean=0.0, inflation_rate_volatility=0.0, initial_balance=100_000.0)
        wm = int(pick(12, 14, 25, 37))
    return Scenario(cls, i, cfgd, wm, int(rng.integers(0, 2 ** 63)), int(rng.integers(2)),
                    int(pick(0, 2 ** 32 - 100, 2 ** 40)), n)


# ---- the oracle's answers, computed once and shared ---------------------------------------------------------------------------
_RUNS = {}


def oracle_run(O, scn: Scenario, wm=None, n=None, trajectories=False, **over):
    """The oracle's `run_batch` of `scn` (with `Config` fields replaced by `over`, at `wm` months, over `n` paths): cached."""
    wm = scn.wm if wm is None else int(wm)
    n = scn.n if n is None else int(n)
    key = (scn.cls, scn.index, scn.seed, scn.begin, scn.cfgd["monthly_expenses"], n, wm, tuple(sorted(over.items())))
    hit = _RUNS.get(key)
    if hit is None or (trajectories and "trajectory" not in hit):
        hit = O.run_batch(scn.params(**over), scn.seed, scn.stream, scn.begin, n, wm, want_trajectories=trajectories)
        _RUNS[key] = hit
    return hit


def oracle_runs(O, jobs, threads: int = 8):
    """`oracle_run(O, *args, **kwargs)` for every `(args, kwargs)` of `jobs`, on host threads (the oracle is a C call)."""
    with ThreadPoolExecutor(max_workers=threads) as pool:
        return list(pool.map(lambda j: oracle_run(O, *j[0], **j[1]), jobs))


def oracle_run_threaded(O, scn: Scenario, threads: int = 16):
    """The integers and summary fields of all of `scn.n` paths without trajectories, the path range cut over host threads."""
    per = (scn.n + threads - 1) // threads
    p = scn.params()

    def work(t):
        b = t * per
        return O.run_batch(p, scn.seed, scn.stream, scn.begin + b, max(0, min(per, scn.n - b)), scn.wm, want_trajectories=False)

    with ThreadPoolExecutor(max_workers=threads) as pool:
        parts = list(pool.map(work, range(threads)))
    return {k: (sum(q[k] for q in parts) if k in ("counters", "ruin_year_bins", "wr_obs_counts") else np.concatenate([q[k] for q in parts]))
            for k in parts[0]}


def money_scale(run) -> float:
    return float(np.abs(run["trajectory"]).max()) if run["trajectory"].size else 0.0


def failure_share(run) -> float:
    return 1.0 - float(run["counters"][0]) / float(run["counters"][1])


def _calibrate(O, scn: Scenario, target: float = 0.5) -> float:
    """Expenses at which about `target` of the paths fail (CAL_STEPS bisection steps at CAL_PATHS paths)."""
    lo, hi = math.log(CAL_LO), math.log(CAL_HI)
    for _ in range(CAL_STEPS):
        mid = 0.5 * (lo + hi)
        c = O.run_batch(scn.params(monthly_expenses=math.exp(mid)), scn.seed, scn.stream, scn.begin, CAL_PATHS, scn.wm, want_trajectories=False)
        if CAL_PATHS - int(c["counters"][0]) > target * CAL_PATHS:
            hi = mid        # more than the target share fail: spend less
        else:
            lo = mid
    return round(math.exp(0.5 * (lo + hi)), 2)


def _fits_a_sliced_launch(scn: Scenario) -> bool:
    frozen = sum(1 for s in scn.cfgd["other_income_streams"] if not s["inflation_indexed"])
    return scn.wm <= 25 and 4 <= scn.cfgd["retirement_years"] <= 8 and frozen <= 2


STATS = {}          # class -> {"drawn", "kept", "dropped_scale", "redrawn_unmixed", "kept_unmixed"}
_KEPT = {}


def _generate(O, cls: str, count: int, sliced_n=None, rng=None, draw=_draw, run_of=None, paths=PATHS, refuse=None):
    """`rng`, `draw`, `run_of`: the generator, the draw and the run a plan is judged by, for plans outside CLASSES (numpy_extra).
    `paths`: the path counts of even / odd indices.  `refuse(scn)`: a further condition on a plan below the money scale, judged
    after its calibration; it returns None, or the name of the STATS counter the plan is redrawn under (never kept)."""
    if rng is None:
        rng = np.random.default_rng([seed(), CLASSES.index(cls), 0 if sliced_n is None else 1])
    if run_of is None:
        run_of = lambda scn: oracle_run(O, scn, n=None if sliced_n is None else SAMPLE, trajectories=True)  # noqa: E731
    stats = {"drawn": 0, "kept": 0, "dropped_scale": 0, "redrawn_unmixed": 0, "kept_unmixed": 0}
    kept = []
    n_of = lambda i: paths[i % 2] if sliced_n is None else sliced_n  # noqa: E731
    while len(kept) < count:
        i = len(kept)
        fallback = None
        for _ in range(MAX_ATTEMPTS):
            scn = draw(cls, rng, i, n_of(i))
            while sliced_n is not None and not _fits_a_sliced_launch(scn):
                scn = draw(cls, rng, i, sliced_n)
            stats["drawn"] += 1
            if stats["drawn"] > 40 * count:
                raise RuntimeError(f"count_fuzz: class {cls} does not yield {count} plans in {40 * count} draws: {stats}")
            scn.cfgd["monthly_expenses"] = _calibrate(O, scn)
            run = run_of(scn)
            if money_scale(run) >= SCALE_LIMIT:
                stats["dropped_scale"] += 1
                continue
            why = refuse(scn) if refuse is not None else None
            if why is not None:
                stats[why] = stats.get(why, 0) + 1
                continue
            fallback = scn
            if MIXED[0] <= failure_share(run) <= MIXED[1]:
                break
            stats["redrawn_unmixed"] += 1
        else:
            if fallback is None:
                continue            # (every attempt was dropped for its scale: draw on, under the cap above)
            scn = fallback          # all-or-nothing after MAX_ATTEMPTS: kept, and counted against the 90 % of the CPU test
            stats["redrawn_unmixed"] -= 1
            stats["kept_unmixed"] += 1
        kept.append(scn)
        stats["kept"] += 1
    return kept, stats


def scenarios(O, cls: str):
    """The kept plans of class `cls` (KEPT[cls] of them), generated once; STATS[cls] says what it took."""
    if cls not in _KEPT:
        _KEPT[cls], STATS[cls] = _generate(O, cls, KEPT[cls])
    return _KEPT[cls]


def sliced_scenario(O, cls: str, n: int):
    """A plan of class `cls` (one of SLICED_CLASSES) that a time-sliced launch of `n` paths takes: working_months <= 25, 4-8
    retirement years, at most two frozen streams (redrawn within the class until that holds); calibrated, and its money scale
    and failure share checked, on a SAMPLE-path trajectory run."""
    return _generate(O, cls, 1, sliced_n=n)[0][0]


# ---- the NumPy leg of a plan: the reference's own random stream, drawn by NumPy itself and injected into the oracle ------------
# rng="numpy" runs path_kernel<MODE, 1, ...> instantiations of its own, and `O.run_batch` has no NumPy generator.  NumPy has: path
# i of a launch at (main_seed, child_offset, stream, path_begin) draws from default_rng(s) with s the first state word of
# SeedSequence(main_seed).spawn(2)[stream].spawn(..)[child_offset + path_begin + i], exactly as the reference's _path_seeds /
# _draw_shock_path do, and the oracle takes the rows through `injected_shocks`.
NUMPY_OFFSETS = (0, 7, 100_000)         # index % 3: the spawn offset an earlier batch of another size leaves behind
NUMPY_BEGINS = (0, 1000)                # (index // 3) % 2
EXTRA = "extra"                         # the class name of numpy_extra's plans
EXTRA_KEPT = 2


def numpy_leg(scn: Scenario):
    """(main_seed, child_offset, path_begin) of plan `scn` on the NumPy stream: the child index of path i is their sum + i."""
    return scn.seed, NUMPY_OFFSETS[scn.index % 3], NUMPY_BEGINS[(scn.index // 3) % 2]


def numpy_path_seeds(scn: Scenario, n=None) -> np.ndarray:
    """The uint32 seed of each of the plan's paths (SeedSequence.spawn appends the child's index to the spawn key)."""
    main, off, begin = numpy_leg(scn)
    n = scn.n if n is None else int(n)
    return np.array([np.random.SeedSequence(main, spawn_key=(scn.stream, off + begin + i)).generate_state(1)[0] for i in range(n)],
                    dtype=np.uint32)


def numpy_shocks(scn: Scenario, wm=None, n=None, rho=None) -> np.ndarray:
    """[n, shock_rows, 3] float64 (equity, inflation, premium): per path default_rng(seed32).standard_normal((shock_rows, 3)),
    then inflation = rho equity + sqrt(max(0, 1 - rho^2)) independent (the reference's _draw_shock_path).  `shock_rows` is the
    oracle's for `wm` months; `rho` is the plan's unless given (an assumption record may move it)."""
    from oracle import oracle as O

    wm = scn.wm if wm is None else int(wm)
    rho = float(scn.cfgd["equity_inflation_correlation"] if rho is None else rho)
    rows = int(O.query_sizes(scn.params(), wm).shock_rows)
    ind = np.stack([np.random.default_rng(int(s)).standard_normal((rows, 3)) for s in numpy_path_seeds(scn, n)])
    out = ind.copy()
    out[:, :, 1] = rho * ind[:, :, 0] + math.sqrt(max(0.0, 1.0 - rho * rho)) * ind[:, :, 1]
    return out


_NUMPY_RUNS = {}


def oracle_run_numpy(O, scn: Scenario, wm=None, n=None, trajectories=False, **over):
    """`oracle_run` on the NumPy stream: the oracle's `run_batch` with `numpy_shocks` injected (cached, apart from the Philox
    runs).  A moved `equity_inflation_correlation` in `over` moves the mix of the shocks with it."""
    wm = scn.wm if wm is None else int(wm)
    n = scn.n if n is None else int(n)
    key = (scn.cls, scn.index, numpy_leg(scn), scn.stream, scn.cfgd["monthly_expenses"], n, wm,
           tuple(sorted((k, repr(v)) for k, v in over.items())))
    hit = _NUMPY_RUNS.get(key)
    if hit is None or (trajectories and "trajectory" not in hit):
        shocks = numpy_shocks(scn, wm, n, over.get("equity_inflation_correlation"))
        hit = O.run_batch(scn.params(**over), 0, scn.stream, 0, n, wm, injected_shocks=shocks, want_trajectories=trajectories)
        _NUMPY_RUNS[key] = hit
    return hit


def oracle_runs_numpy(O, jobs, threads: int = 8):
    """`oracle_run_numpy(O, *args, **kwargs)` for every `(args, kwargs)` of `jobs`, on host threads."""
    with ThreadPoolExecutor(max_workers=threads) as pool:
        return list(pool.map(lambda j: oracle_run_numpy(O, *j[0], **j[1]), jobs))


def _draw_extra(cls, rng, i, n):
    """The one family CLASSES leave out: the generic variant for its 17-20 paying streams WITH an annual-gains tax on one asset
    (asset 1 for even i, asset 2 for odd i).  The rest is a `generic` plan of even index 2 i: rho = 0, then rho = +-1."""
    scn = _draw("generic", rng, 2 * i, n)
    a = ("inv1", "inv2")[i % 2]
    scn.cfgd.update({"scenario": f"{cls}-{i}", f"{a}_use_realized_gains_tax_system": False,
                     f"{a}_annual_tax_on_gains_rate": float(rng.uniform(0.05, 0.5))})
    scn.cls, scn.index = cls, i
    return scn


def numpy_extra(O):
    """EXTRA_KEPT plans of class EXTRA, from a generator of their own (no plan of CLASSES moves); calibrated as the classes'
    plans are, and judged (money scale, mixed outcomes) by their run on the NumPy stream, the one they are for."""
    if EXTRA not in _KEPT:
        _KEPT[EXTRA], STATS[EXTRA] = _generate(O, EXTRA, EXTRA_KEPT, rng=np.random.default_rng([seed(), len(CLASSES), 2]),
                                               draw=_draw_extra, run_of=lambda scn: oracle_run_numpy(O, scn, trajectories=True))
    return _KEPT[EXTRA]


def numpy_plans(O, cls: str):
    """The plans of `cls` on the NumPy stream: a class of CLASSES, or EXTRA."""
    return numpy_extra(O) if cls == EXTRA else scenarios(O, cls)


# ---- the SCREENED family: plans a count-only launch screens in fp32 (csrc/mcr_screen.h) ---------------------------------------
# The classes' plans rarely qualify for the screened route (half their income records are frozen-nominal), and the tests that
# run them address the classic kernels.  These plans are drawn for that route: `_draw` of one of five tax BASES supplies the
# market (rho strata, volatilities outside the narrow exp window, the last rate below the exact month), the months, the seed
# and the path range (2^32 - 100 and 2^40 among them); the income records, the allocation and the initial balance are drawn
# here, as strata of the plan's index within its base:
#
#     index % 3:       0, 1 or 2 paying, inflation-indexed income records (SCREENED_FEATURES: what their draw must reach)
#     index odd:       a record that pays nothing, frozen-nominal allowed, at a random list position (the kernel is not given it)
#     index % 4 == 3:  an EDGE plan: allocation 0, allocation 1 or initial balance 0 in turn: every path is DOUBTFUL by
#                      construction (a balance at or below one dollar), so the fp64 re-run gets the whole, ragged range
#     otherwise:       INTERIOR: allocation uniform in (0.05, 0.95), initial balance log-uniform in [1e3, 1e6]
#     index even:      15-40 retirement years (odd: `_draw`'s 4-40; the short ones have few SAFE paths, or none)
#
# Each plan has two expense LEVELS, calibrated with the oracle alone: "half" (half the paths fail: a long list of doubtful
# paths) and "comfortable" (5 % fail: most paths SAFE, a short list).  A plan is dropped for its money scale and redrawn for
# all-or-nothing outcomes as the classes' plans are, both judged at the "half" level; it is also redrawn unless it takes the
# screened route at a million paths with no knob set, and unless its tolerance (`screen_reference`) is at most SCREENED_TOL_MAX
# at both levels.  A generator of its own per base: no plan of CLASSES or of numpy_extra moves.
SCREENED_BASES = ("equal_rates", "unequal_rates", "mask1", "mask2", "mask0")
SCREENED_KEPT = 8
SCREENED_PATHS = (1025, 705)            # even / odd index: four screening workgroups and one lane; two, three wavefronts and one lane
SCREENED_LEVELS = {"half": 0.5, "comfortable": 0.05}
SCREENED_EDGES = ("allocation 0", "allocation 1", "initial balance 0")
SCREENED_FEATURES = ("starts before retirement", "duration 0", "no duration", "tax rate 1")
SCREENED_TOL_FLOOR, SCREENED_TOL_FACTOR, SCREENED_TOL_MAX = 2e-4, 8.0, 1e-2
SCREEN_KNOBS = ("MCR_K1_SCREEN", "MCR_K1_SCREEN_MIN_PATHS", "MCR_K1_SCREEN_EXPECTED", "MCR_K1_RERUN_PRODUCERS", "MCR_K1_SPLIT_MAX_WAVES",
                "MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS", "MCR_K1_SEGMENT_ORDER", "MCR_K1_GROWTH_FORM",
                "MCR_K1_MONTH_FORM", "MCR_K1_STREAM_FORM")


def screened_class(base: str) -> str:
    return f"screened-{base}"


def screened_edge(scn: Scenario):
    """The edge of an edge plan (one of SCREENED_EDGES), None for an interior plan."""
    if scn.index % 4 != 3:
        return None
    return SCREENED_EDGES[(2 * SCREENED_BASES.index(scn.cls[len("screened-"):]) + scn.index // 4) % 3]


def screened_features(scn: Scenario):
    """Which of SCREENED_FEATURES the plan's PAYING income records show."""
    retirement = scn.cfgd["current_age"] + scn.wm / 12.0
    out = set()
    for s in scn.cfgd["other_income_streams"]:
        if s["monthly_amount_today"] == 0.0:
            continue
        out |= {f for f, holds in zip(SCREENED_FEATURES, (s["start_at_age"] < retirement, s["duration_years"] == 0,
                                                          s["duration_years"] is None, s["tax_rate"] == 1.0)) if holds}
    return out


def _draw_screened(cls, rng, i, n):
    base = cls[len("screened-"):]
    scn = _draw(base, rng, i, n)
    pick = lambda *xs: xs[int(rng.integers(len(xs)))]  # noqa: E731
    retirement = scn.cfgd["current_age"] + scn.wm / 12.0
    records = []
    for s in range(i % 3):
        rec = {"name": f"s{s}", "monthly_amount_today": float(rng.uniform(50, 4000)),
               "start_at_age": float(retirement + pick(-rng.uniform(0.1, 10), rng.uniform(0, 25), rng.uniform(0, 10))),
               "duration_years": pick(None, 0, int(rng.integers(1, 12)), int(rng.integers(1, 12))), "inflation_indexed": True,
               "tax_rate": float(pick(0.0, 1.0, rng.uniform(0, 0.6), rng.uniform(0, 0.6)))}
        if s == 0:      # the first record shows one feature for certain, in turn over the base's plans and over the bases
            forced = SCREENED_FEATURES[(i // 3 + SCREENED_BASES.index(base)) % 4]
            rec.update({"starts before retirement": {"start_at_age": float(retirement - rng.uniform(0.1, 10))}, "duration 0": {"duration_years": 0},
                        "no duration": {"duration_years": None}, "tax rate 1": {"tax_rate": 1.0}}[forced])
        records.append(rec)
    if i % 2 == 1:
        records.insert(int(rng.integers(len(records) + 1)),
                       {"name": "nothing", "monthly_amount_today": 0.0, "start_at_age": float(retirement + rng.uniform(-3, 25)),
                        "duration_years": pick(None, int(rng.integers(0, 12))), "inflation_indexed": bool(rng.integers(2)),
                        "tax_rate": float(rng.uniform(0, 0.6))})
    alloc, balance = float(rng.uniform(0.05, 0.95)), float(math.exp(rng.uniform(math.log(1e3), math.log(1e6))))
    scn.cls = cls
    scn.cfgd.update(scenario=f"{cls}-{i}", other_income_streams=records, allocation_inv1_pct=alloc, initial_balance=balance)
    if i % 2 == 0:      # (a retirement of 4-8 years has no SAFE path at the "half" level: 24 months of need are a large part of it)
        scn.cfgd["retirement_years"] = int(rng.integers(15, 41))
    edge = screened_edge(scn)
    if edge is not None:
        scn.cfgd.update({"allocation 0": {"allocation_inv1_pct": 0.0}, "allocation 1": {"allocation_inv1_pct": 1.0},
                         "initial balance 0": {"initial_balance": 0.0}}[edge])
    return scn


def at_level(scn: Scenario, level: str) -> Scenario:
    """The plan at one of its two expense levels (a copy: `scn` itself stands at "half")."""
    out = Scenario(scn.cls, scn.index, dict(scn.cfgd, monthly_expenses=scn.levels[level]), scn.wm, scn.seed, scn.stream, scn.begin, scn.n)
    out.levels = scn.levels
    return out


_SCREEN_REFERENCES = {}


def screen_reference(scn: Scenario, level: str):
    """The reference of plan `scn` at `level` (tests/screen_model.py: the screening kernel's loop in plain NumPy), cached:
    `fp64` and `fp32`, the model's run in either precision; `dev`, the largest relative deviation of the fp32 run from the fp64
    one over `min_ratio` and `final_total` of the paths SAFE in both (0.0 without such a path); and the plan's tolerance
    `tol` = max(SCREENED_TOL_FLOOR, SCREENED_TOL_FACTOR dev), measured from the reference and never from the kernel.  The
    factor: NumPy's single-precision exp and log are within an ulp, while the kernel adds about 1e-6 absolute on each normal
    (csrc/mcr_screen.h) and a few ulp on each hardware exp, log and reciprocal."""
    import screen_model

    key = (scn.cls, scn.index, scn.seed, scn.begin, scn.n, scn.wm, scn.levels[level])
    if key not in _SCREEN_REFERENCES:
        s = at_level(scn, level)
        fp64, fp32 = (screen_model.model(s.params(), s.cfgd, s.wm, s.seed, s.stream, s.begin, s.n, dtype=t) for t in (np.float64, np.float32))
        both = fp64["safe"] & fp32["safe"]
        dev = 0.0
        for k in ("min_ratio", "final_total"):
            a, b = fp64[k][both], fp32[k][both].astype(np.float64)
            finite = np.isfinite(a)
            if not np.array_equal(finite, np.isfinite(b)):      # (a month has a need in one precision only: no tolerance covers that)
                dev = math.inf
            elif finite.any():
                dev = max(dev, float(np.abs(b[finite] / a[finite] - 1.0).max()))
        _SCREEN_REFERENCES[key] = {"fp64": fp64, "fp32": fp32, "dev": dev, "tol": max(SCREENED_TOL_FLOOR, SCREENED_TOL_FACTOR * dev)}
    return _SCREEN_REFERENCES[key]


def _takes_the_screened_route(scn: Scenario) -> bool:
    from monte_carlo_retirement_amd import engine as E

    old = {k: os.environ.pop(k, None) for k in SCREEN_KNOBS}
    try:
        return E.screen(scn.params(), scn.wm, 10 ** 6)
    finally:
        os.environ.update({k: v for k, v in old.items() if v is not None})


def screened_scenarios(O, base: str):
    """The SCREENED_KEPT kept plans of base `base` (one of SCREENED_BASES), generated once: each stands at its "half" level,
    and `scn.levels` holds both.  STATS[screened_class(base)] says what it took."""
    cls = screened_class(base)
    if cls not in _KEPT:
        def refuse(scn):
            if not _takes_the_screened_route(scn):
                return "redrawn_unqualified"
            scn.levels = {"half": scn.cfgd["monthly_expenses"], "comfortable": _calibrate(O, scn, SCREENED_LEVELS["comfortable"])}
            if max(screen_reference(scn, level)["tol"] for level in SCREENED_LEVELS) > SCREENED_TOL_MAX:
                return "redrawn_tolerance"
            return None

        _KEPT[cls], STATS[cls] = _generate(O, cls, SCREENED_KEPT, rng=np.random.default_rng([seed(), len(CLASSES) + 1, SCREENED_BASES.index(base)]),
                                           draw=_draw_screened, paths=SCREENED_PATHS, refuse=refuse)
        for k in ("redrawn_unqualified", "redrawn_tolerance"):
            STATS[cls].setdefault(k, 0)
    return _KEPT[cls]
