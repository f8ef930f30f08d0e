"""Random plans for the spending-rule kernels, with the CPU model's answer to each: a helper, not a test.

The rule kernels (`mcr_run_rule_rng`, the rule yearly bins, the rule fan-out and the rule grid fan-out) run the generic tax mask
for every plan they accept, and their oracle-backed tests run three hand-made plans.  Here they get the stratified random plans
of tests/count_fuzz.py: the first PER_CLASS kept plans of each class of CLASSES (every class but `generic`, which the rule
launch refuses: more than 16 income streams, the exact month), unchanged, at the suite's seed, with their own working months,
seed, stream, first path (0, 2^32 - 100, 2^40) and path count (512 / 321).  A plan runs under rule RULE_NAMES[index % 5], `index`
the plan's index within its class (count_fuzz's strata are functions of it too: rho by index % 5, so each class meets the rules
on another market by its own draws); case k (0 .. 35) counts the plans class by class.

The plans' `monthly_expenses` were calibrated for fixed spending; under a rule they are calibrated again, on the CPU alone
(`spending_rule_model.model`, i.e. the unmodified oracle): CAL_STEPS bisection steps on log-expenses over count_fuzz's
[CAL_LO, CAL_HI] at CAL_PATHS paths, towards half the paths failing on even indices and one fifth on odd ones (a plan that
fails seldom is one whose balances outgrow the upper guardrail: that is what makes raises occur).

`answer(O, case)` is the CPU model's answer to a case, computed once and shared: per path the model's multiplier row and the
oracle's run of it, and from those the success count, the year counts and the YearsToRuin column.  STATS keeps what the family
looks like (tests/test_rule_fuzz_cpu.py asserts it is worth running, and prints it).
"""

from __future__ import annotations

import math
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

import count_fuzz as F
import spending_rule_model as M

CLASSES = ("equal_rates", "unequal_rates", "mask1", "mask2", "mask0", "annual")
PER_CLASS = 6
#: (upper, lower, cut, raise, floor, ceiling); `always`: every year decides; `pinned`: decisions fire every year, yet m can only be 1
RULES = {"symmetric": (1.2, 0.8, 0.10, 0.10, 0.5, 1.5),
         "always": (1.0, 1.0, 0.25, 0.30, 0.0, 3.0),
         "cut_only": (1.0, 0.0, 0.10, 0.0, 0.6, 1.0),
         "generous": (1.5, 0.9, 0.05, 0.20, 0.7, 2.0),
         "pinned": (1.0, 1.0, 0.5, 1.0, 1.0, 1.0)}
RULE_NAMES = tuple(RULES)
CAL_PATHS, CAL_STEPS = 64, F.CAL_STEPS
TARGETS = (0.5, 0.2)                    # even / odd plan index:the share of the calibration paths that fail
THREADS = 8                             # host threads over a case's paths (the oracle is a C call)


@dataclass
class Case:
    k: int                              # 0 .. len(CLASSES) * PER_CLASS - 1
    scn: F.Scenario                     # a copy of count_fuzz's plan at the level calibrated under the rule
    rname: str
    level: float

    @property
    def rule(self):
        return RULES[self.rname]

    @property
    def id(self) -> str:
        return f"{self.k:02d}-{self.scn.cls}-{self.scn.index}-{self.rname}"

    def params(self, **over):
        return self.scn.params(**over)

    def at(self, **over) -> "Case":
        """The case with `Config` fields of its plan replaced (another level, other amounts), or `rname` / `wm`."""
        rname, wm = over.pop("rname", self.rname), over.pop("wm", self.scn.wm)
        s = self.scn
        scn = F.Scenario(s.cls, s.index, dict(s.cfgd, **over), int(wm), s.seed, s.stream, s.begin, s.n)
        return Case(self.k, scn, rname, float(scn.cfgd["monthly_expenses"]))

    def context(self, route: str = "") -> str:
        return f"case {self.id} rule {self.rname} = {self.rule}: " + self.scn.context(route)


STATS = {"levels": {}, "cases": {}, "seconds": {}}        # case id -> calibrated level / the counts of `answer` / generation time per class
_CASES = {}
_ANSWERS = {}


def _paths(fn, n):
    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        return list(pool.map(fn, range(n)))


def calibrate(scn: F.Scenario, rule, target: float) -> float:
    """Expenses at which about `target` of the first CAL_PATHS paths of `scn` fail UNDER `rule`, by the CPU model alone."""
    lo, hi = math.log(F.CAL_LO), math.log(F.CAL_HI)
    for _ in range(CAL_STEPS):
        mid = 0.5 * (lo + hi)
        p = scn.params(monthly_expenses=math.exp(mid))
        failed = sum(_paths(lambda i: not bool(M.model(p, scn.wm, rule, scn.seed, scn.stream, scn.begin + i)[1]["success"][0]), CAL_PATHS))
        if failed > target * CAL_PATHS:
            hi = mid        # more than the target share fail: spend less
        else:
            lo = mid
    return round(math.exp(0.5 * (lo + hi)), 2)


def _generate(O, cls: str, count: int = PER_CLASS):
    base = CLASSES.index(cls) * PER_CLASS
    out = []
    for s in F.scenarios(O, cls)[:count]:
        k = base + s.index
        rname = RULE_NAMES[s.index % len(RULE_NAMES)]
        level = calibrate(s, RULES[rname], TARGETS[s.index % 2])
        scn = F.Scenario(s.cls, s.index, dict(s.cfgd, monthly_expenses=level), s.wm, s.seed, s.stream, s.begin, s.n)
        out.append(Case(k, scn, rname, level))
    return out


def cases(O, cls: str):
    """The PER_CLASS cases of class `cls` (one of CLASSES), generated once."""
    if cls not in _CASES:
        t0 = time.time()
        _CASES[cls] = _generate(O, cls)
        STATS["seconds"][cls] = round(time.time() - t0, 1)
        for c in _CASES[cls]:
            STATS["levels"][c.id] = c.level
    return _CASES[cls]


def case(O, cls: str, index: int) -> Case:
    return cases(O, cls)[index]


def all_cases(O):
    return [c for cls in CLASSES for c in cases(O, cls)]


TIES = ((0, 1.0), (13, 0.0), (12, 1.0))        # (working months, allocation_inv1_pct) of the tie cases
TIE_PATHS, TIE_BEGIN, TIE_YEARS = 130, 2 ** 32 - 3, 9


def tie_cases(O):
    """Hand-made cases where the rule's comparison is an EXACT tie every year, under `always` (upper = lower = 1: a year that
    does not tie is cut or raised).  A flat market (every mean and volatility 0), one asset only, nothing spent: the balance
    stays at its start value to the bit and the price level at 1.0, so (m r0) P == upper B == lower B.  The rule cuts on
    `>` and raises on `<` (include/mcr.h), so m stays 1; a kernel that compares with `>=` cuts every year.  No random plan
    reaches a tie, and `verify` calls a tie undecidable: what holds these cases is the model's row, bit for bit."""
    s = F.scenarios(O, "mask0")[0]
    out = []
    for j, (wm, alloc) in enumerate(TIES):
        cfgd = dict(s.cfgd, scenario=f"tie-{j}", monthly_expenses=0.0, initial_balance=250_000.0, monthly_contribution=100.0,
                    contribution_growth_rate_annual=0.0, allocation_inv1_pct=alloc, retirement_years=TIE_YEARS, other_income_streams=[],
                    inv1_returns_mean=0.0, inv1_returns_volatility=0.0, inv2_premium_over_inflation_mean=0.0,
                    inv2_premium_over_inflation_volatility=0.0, inflation_rate_mean=0.0, inflation_rate_volatility=0.0,
                    equity_inflation_correlation=0.0, inv1_use_realized_gains_tax_system=True, inv1_realized_gains_tax_rate=0.2,
                    inv2_use_realized_gains_tax_system=True, inv2_realized_gains_tax_rate=0.3)
        out.append(Case(1000 + j, F.Scenario("tie", j, cfgd, wm, s.seed, s.stream, TIE_BEGIN, TIE_PATHS), "always", 0.0))
    return out


def answer(O, c: Case):
    """The CPU model's answer to case `c`, cached and read only: ``rows`` ``[ry, n]`` (the model's multipliers, NaN for a year a
    path does not begin), ``runs`` (per path the oracle's run of the model's final schedule), ``success`` (bool ``[n]``),
    ``years_to_ruin`` and ``final_balance`` ``[n]``, ``successes``, ``year_counts`` ``[ry, 4]``."""
    if c.id not in _ANSWERS:
        p, s = c.params(), c.scn
        got = _paths(lambda i: M.model(p, s.wm, c.rule, s.seed, s.stream, s.begin + i), s.n)
        rows = np.stack([row for row, _ in got], axis=1)
        runs = [run for _, run in got]
        success = np.array([bool(r["success"][0]) for r in runs])
        ytr = np.array([float(r["years_to_ruin"][0]) for r in runs])
        counts = M.year_counts_of(rows, c.rule)
        _ANSWERS[c.id] = {"rows": rows, "runs": runs, "success": success, "years_to_ruin": ytr,
                          "final_balance": np.array([float(r["final_balance"][0]) for r in runs]),
                          "successes": int(success.sum()), "year_counts": counts}
        STATS["cases"][c.id] = {"level": c.level, "paths": s.n, "begin": s.begin, "wm": s.wm, "failed": int(s.n - success.sum()),
                                "begun": int(counts[:, 0].sum()), "cut": int(counts[:, 1].sum()), "floor": int(counts[:, 2].sum()),
                                "raised": int(counts[:, 3].sum()), "pre_retirement": int(np.count_nonzero(ytr == 0.0))}
    return _ANSWERS[c.id]


def outcome(res, i: int) -> dict:
    """Path i of a summary launch (or of `answer`) as `spending_rule_model.verify` takes it."""
    return {"success": res["success"][i], "years_to_ruin": res["years_to_ruin"][i], "final_balance": res["final_balance"][i]}


def verify_rows(c: Case, rows, res):
    """`spending_rule_model.verify` of every path of case `c` against multiplier rows ``[ry, n]`` and the outcome columns of
    `res`: raises AssertionError with the case's context; returns the bool ``[n]`` of paths with an undecidable year."""
    p, s = c.params(), c.scn

    def one(i):
        try:
            return M.verify(p, s.wm, c.rule, s.seed, s.stream, s.begin + i, rows[:, i], outcome(res, i))
        except AssertionError as e:
            raise AssertionError(f"{e.args}: path {s.begin} + {i}: {c.context('verify')}") from e

    return np.array(_paths(one, s.n), dtype=bool)
