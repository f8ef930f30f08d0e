"""The plans tests/count_fuzz.py generates are worth running: mixed outcomes, few dropped for their money scale, every class
filled, and every compiled count-only variant of the path kernel (tax masks 0-3, growth masks 0 / 1 / 3, month form 1, the
pre-retirement failures of the annual-gains kernels, the last rate below the exact-month switch) reached by some plan.  The
generator, the CPU oracle and the host's form choice (mcr_k1_growth_form / mcr_k1_month_form) only: no device needed."""

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
