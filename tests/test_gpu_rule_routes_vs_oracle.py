"""Every spending-rule kernel against the CPU oracle, on the random cases of tests/rule_fuzz.py.

The other tests of these kernels run three plans derived from scenarios/config.json on paths 0 .. 599 of one seed under two
firing rules; the kernels run the generic tax mask for every plan they accept, so no test had put one asset realized and the
other annual, an untaxed asset, a rate just below the exact-month switch, an allocation of 0 or 1, rho = 0 or +-1, a zero
volatility, income streams that start mid-year, a 7-year retirement, working months 1 / 11 / 13 / 25, stream 0, or a path range
across the 32-bit word of the Philox counter under a rule.  The 36 cases of rule_fuzz do (five rules, among them one where every
year decides and one that decides and can only keep m = 1).

a. the summary launch (MODE 1) with multiplier rows: `spending_rule_model.verify` of every path (the oracle's run of the GPU's
   own schedule gives the GPU's outcome; every multiplier is the rule's decision on the oracle's sample), and where no year is
   undecidable the row is the CPU model's bit for bit; b. the count-only launch (MODE 0); c. two launches over a split range;
d. the rule fan-out (PHASE 11) and its outcome rows; e. the rule grid fan-out (PHASE 6 with RULE); f. the rule yearly bins (MODE 3
with RULE).  d, e and f are held to a's and b's launches, integers and bit patterns; each runs on every third case.  Tolerances:
`verify`'s (test_gpu_differential.ABS / REL); at most 1 % of a case's paths may have an undecidable year (the cap of
test_gpu_spending_rule.py).  The balance tables of f are left to test_gpu_rule_year_bins.test_firing_rules_vs_the_oracle, whose
treatment of samples near an edge is part of that test's body."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import count_fuzz as F
import rule_fuzz as RF
import spending_rule_model as M
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.spending_rules import SpendingRule
from test_gpu_rule_year_bins import EDGES, WR_EDGES, _check_against_rule_launch     # that file's comparison of the tables with the rule launch

pytestmark = pytest.mark.gpu
CASES = [(cls, i) for cls in RF.CLASSES for i in range(RF.PER_CLASS)]
IDS = [f"{cls}-{i}" for cls, i in CASES]
KNOBS = ("MCR_RULE_FANOUT_MIN_WAVES", "MCR_EXPENSE_FANOUT_MIN_WAVES", "MCR_K1_LDS_LOCK_SLOTS")
FACTORS = (0.7, 1.0, 1.15)
SENTINEL = -7
_summaries = {}


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _every_third(offset):
    """Every third plan of each class, the start moving on by one from class to class: with six plans and five rules per class
    a fixed start would give a route the same two rules in every class."""
    picked = [(x, i) for x, i in zip(CASES, IDS) if (RF.CLASSES.index(x[0]) + x[1]) % 3 == offset]
    return pytest.mark.parametrize("cls,index", [x for x, _ in picked], ids=[i for _, i in picked])


def _rule(c, rname=None):
    return SpendingRule(*RF.RULES[rname or c.rname])


def _launch(c, want="count", begin=None, n=None, **kw):
    s = c.scn
    return E.run_rule_host(c.params(), s.seed, s.stream, s.begin if begin is None else begin, s.n if n is None else n, s.wm, _rule(c), want=want, **kw)


def _summary(c):
    """a's launch of a case, run once and shared (read only)."""
    if c.id not in _summaries:
        _summaries[c.id] = _launch(c, want="summary", multipliers=True)
    return _summaries[c.id]


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint8)


# ---- a, b, c: the plain rule launch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,index", CASES, ids=IDS)
def test_the_rule_launch_follows_the_oracle(oracle, cls, index):
    c = RF.case(oracle, cls, index)
    s, ry = c.scn, int(c.scn.cfgd["retirement_years"])
    cpu = RF.answer(oracle, c)
    got = _summary(c)
    rows = got["multipliers"]
    assert rows.shape == (ry, s.n), c.context("summary")
    # a. every path against the oracle's run of the GPU's own schedule
    undecidable = RF.verify_rows(c, rows, got)
    print(f"{c.id}: undecidable paths {int(undecidable.sum())} of {s.n}; failed {s.n - int(got['counters'][0])} (CPU model {s.n - cpu['successes']})")
    assert undecidable.sum() <= 0.01 * s.n, (int(undecidable.sum()), c.context("summary"))
    counts = M.year_counts_of(rows, c.rule)
    assert np.array_equal(got["year_counts"].astype(np.int64), counts), c.context("summary: year_counts")
    assert got["counters"].astype(np.int64).tolist() == [int(got["success"].sum()), s.n], c.context("summary: counters")
    sure = ~undecidable
    assert np.array_equal(_bits(rows[:, sure]), _bits(cpu["rows"][:, sure])), c.context("summary: rows of decidable paths")
    assert np.array_equal(got["success"].astype(bool)[sure], cpu["success"][sure]), c.context("summary: success of decidable paths")
    assert np.array_equal(got["years_to_ruin"][sure], cpu["years_to_ruin"][sure], equal_nan=True), c.context("summary: years_to_ruin")
    if not undecidable.any():
        assert np.array_equal(counts, cpu["year_counts"]) and int(got["counters"][0]) == cpu["successes"], c.context("summary: the model's counts")
    if c.rname == "pinned":         # decisions fire every year and change nothing: the plain launch, bit for bit
        plain = E.run_batch_host(c.params(), s.seed, s.stream, s.begin, s.n, s.wm, want_trajectories=False, want_bins=False)
        assert got["counters"].tolist() == plain["counters"].tolist(), c.context("pinned: counters")
        for k in E.SUMMARY_FIELDS + ("success",):
            assert np.array_equal(_bits(got[k]), _bits(plain[k])), (k, c.context("pinned"))
        assert np.all((rows == 1.0) | np.isnan(rows)), c.context("pinned: rows")
    # b. count-only (MODE 0)
    count = _launch(c)
    assert set(count) == {"counters", "year_counts"}
    assert count["counters"].tolist() == got["counters"].tolist(), c.context("count-only: counters")
    assert np.array_equal(count["year_counts"], got["year_counts"]), c.context("count-only: year_counts")
    # c. two launches: at the 32-bit word of the counter where the range crosses it, else at an odd path
    first = 100 if s.begin == 2 ** 32 - 100 else 333 if s.n == 512 else 129
    assert s.begin != 2 ** 32 - 100 or s.begin + first == 2 ** 32
    parts = [_launch(c, want="summary", begin=s.begin + b, n=n, multipliers=True) for b, n in ((0, first), (first, s.n - first))]
    assert np.array_equal(_bits(np.concatenate([x["multipliers"] for x in parts], axis=1)), _bits(rows)), c.context(f"partition at {first}: rows")
    assert np.array_equal(parts[0]["year_counts"] + parts[1]["year_counts"], got["year_counts"]), c.context(f"partition at {first}: year_counts")
    assert (parts[0]["counters"] + parts[1]["counters"]).tolist() == got["counters"].tolist(), c.context(f"partition at {first}: counters")
    for k in E.SUMMARY_FIELDS + ("success",):
        assert np.array_equal(_bits(np.concatenate([x[k] for x in parts])), _bits(got[k])), (k, c.context(f"partition at {first}"))
    parts = [_launch(c, begin=s.begin + b, n=n) for b, n in ((0, first), (first, s.n - first))]
    assert np.array_equal(parts[0]["year_counts"] + parts[1]["year_counts"], got["year_counts"]), c.context(f"count-only partition at {first}")
    assert (parts[0]["counters"] + parts[1]["counters"]).tolist() == got["counters"].tolist(), c.context(f"count-only partition at {first}")


# ---- d. the rule fan-out ---------------------------------------------------------------------------------------------------------
def _options(c):
    """17 options, two fan-out launches of unequal groups (9 + 8) where a launch takes MCR_MAX_EXPENSE_FANOUT of them: the case's
    own rule at 0.7 x, 1 x and 1.15 x its level, the other four rules at 1 x, fixed spending (None), the case's rule with the
    initial balance and the contribution moved; and the other four rules at 0.7 x and 1.15 x.  Option 1 is the case itself."""
    cfg = c.scn.cfgd
    b0, c0 = float(cfg["initial_balance"]), float(cfg["monthly_contribution"])
    others = [r for r in RF.RULE_NAMES if r != c.rname]
    options = [(b0, c0, c.level * f, c.rname) for f in FACTORS]
    options += [(b0, c0, c.level, r) for r in others]
    options += [(b0, c0, c.level, None), (b0 * 1.25 + 1000.0, c0 * 0.5 + 10.0, c.level, c.rname)]
    options += [(b0, c0, c.level * f, r) for r in others for f in (FACTORS[0], FACTORS[2])]
    assert len(options) == 17
    return options


@_every_third(0)
def test_the_rule_fan_out_counts_what_the_rule_launches_count(oracle, cls, index):
    import torch

    c = RF.case(oracle, cls, index)
    s = c.scn
    options = _options(c)
    records = [(b, k, e, None if r is None else _rule(c, r)) for b, k, e, r in options]
    # per option the count-only rule launch of the option's plan under its rule (fixed spending: the neutral rule)
    want = [E.run_rule_host(s.params(initial_balance=b, monthly_contribution=k, monthly_expenses=e), s.seed, s.stream, s.begin, s.n, s.wm,
                            SpendingRule.neutral() if r is None else _rule(c, r)) for b, k, e, r in options]
    assert not want[7]["year_counts"][:, 1:].any(), c.context("fixed spending")
    counts, years = E.probe_rules(c.params(), s.seed, s.stream, s.begin, s.n, s.wm, records)
    launches = int(N.load_library().mcr_probe_rules_last_fanout_launches())
    print(f"{c.id}: rule fan-out launches {launches} for {len(options)} options, {s.frozen_streams()} frozen streams")
    assert launches >= 2, c.context("rule fan-out")
    counts, years = counts.cpu().numpy(), years.cpu().numpy()
    for k, w in enumerate(want):
        assert counts[k].tolist() == w["counters"].astype(np.int64).tolist(), (k, options[k], c.context("rule fan-out: counters"))
        assert np.array_equal(years[k], w["year_counts"].astype(np.int64)), (k, options[k], c.context("rule fan-out: year_counts"))
    a = _summary(c)
    assert counts[1].tolist() == a["counters"].astype(np.int64).tolist(), c.context("rule fan-out: the case's own option")
    assert np.array_equal(years[1], a["year_counts"].astype(np.int64)), c.context("rule fan-out: the case's own option")
    # the outcome rows: where(success, final_balance, NaN) and years_to_ruin of the summary launch, bit for bit; nothing beyond n
    stride = 640
    dev = torch.device("cuda", 0)
    fin = torch.full((len(records), stride), float(SENTINEL), dtype=torch.float64, device=dev)
    ruin = torch.full((len(records), stride), float(SENTINEL), dtype=torch.float64, device=dev)
    counts2, years2, _, _ = E.probe_rules_outcomes(c.params(), s.seed, s.stream, s.begin, s.n, s.wm, records, final_balance=fin, years_to_ruin=ruin,
                                                   path_stride=stride)
    fin, ruin = fin.cpu().numpy(), ruin.cpu().numpy()
    assert np.array_equal(counts2.cpu().numpy(), counts) and np.array_equal(years2.cpu().numpy(), years), c.context("rule fan-out outcomes: counts")
    want_final = np.where(a["success"].astype(bool), a["final_balance"], np.nan)
    assert np.array_equal(_bits(fin[1, :s.n]), _bits(want_final)), c.context("rule fan-out outcomes: final_balance")
    assert np.array_equal(_bits(ruin[1, :s.n]), _bits(a["years_to_ruin"])), c.context("rule fan-out outcomes: years_to_ruin")
    assert np.all(fin[:, s.n:] == SENTINEL) and np.all(ruin[:, s.n:] == SENTINEL), c.context("rule fan-out outcomes: beyond n")
    assert np.array_equal(np.count_nonzero(~np.isnan(fin[:, :s.n]), axis=1), counts[:, 0]), c.context("rule fan-out outcomes: successes")


# ---- e. the rule grid fan-out ------------------------------------------------------------------------------------------------------
@_every_third(1)
def test_the_rule_grid_counts_what_the_rule_launches_count(oracle, cls, index):
    c = RF.case(oracle, cls, index)
    s = c.scn
    months = [s.wm, s.wm + 1, s.wm + 12]
    levels = [[c.level * f for f in FACTORS] for _ in months]
    counts, years = E.probe_rule_grid(c.params(), s.seed, s.stream, s.begin, s.n, months, levels, _rule(c))
    launches = int(N.load_library().mcr_probe_rule_grid_last_fanout_launches())
    print(f"{c.id}: rule grid fan-out launches {launches} (0: the per-row route) for months {months}, {s.frozen_streams()} frozen streams")
    counts, years = counts.cpu().numpy(), years.cpu().numpy()
    for r, wm in enumerate(months):
        for k, level in enumerate(levels[r]):
            w = _launch(c.at(monthly_expenses=level, wm=wm))
            assert counts[r, k].tolist() == w["counters"].astype(np.int64).tolist(), (wm, level, launches, c.context("rule grid: counters"))
            assert np.array_equal(years[r, k], w["year_counts"].astype(np.int64)), (wm, level, launches, c.context("rule grid: year_counts"))
    a = _summary(c)
    assert counts[0, 1].tolist() == a["counters"].astype(np.int64).tolist(), c.context("rule grid: the case's own cell")
    assert np.array_equal(years[0, 1], a["year_counts"].astype(np.int64)), c.context("rule grid: the case's own cell")


# ---- f. the rule yearly bins ---------------------------------------------------------------------------------------------------------
@_every_third(2)
def test_the_rule_yearly_bins_are_the_rule_launch(oracle, cls, index):
    import torch

    c = RF.case(oracle, cls, index)
    s = c.scn
    p = c.params()
    a = _summary(c)
    sz = E.query_sizes(p, s.wm)
    dev = torch.device("cuda", 0)
    wr_obs = torch.zeros(sz.retirement_years, dtype=torch.int64, device=dev)
    ruin = torch.zeros(sz.ruin_bins, dtype=torch.int64, device=dev)
    E.run_rule(p, s.seed, s.stream, s.begin, s.n, s.wm, _rule(c), out_extra={"wr_obs_counts": wr_obs.data_ptr(), "ruin_year_bins": ruin.data_ptr()})
    cnt = {"counters": a["counters"], "year_counts": a["year_counts"], "wr_obs_counts": wr_obs.cpu().numpy().astype(np.uint64),
           "ruin_year_bins": ruin.cpu().numpy().astype(np.uint64)}
    # The default edges (256 + 256 + 64 bins) leave the lock columns of two frozen income streams beside them in the LDS of four
    # resident workgroups; a plan with more is refused by name (include/mcr.h: "frozen streams beyond the LDS budget"; the rule
    # kernels have no generic variant to fall back to) and runs on the 64-bin edges of test_gpu_rule_year_bins.py instead.  A plan
    # without a frozen stream can never be refused for them.
    edge_sets = [("default edges", {}), ("64-bin edges", {"edges": EDGES, "wr_edges": WR_EDGES})]
    for name, kw in edge_sets:
        try:
            yb = E.run_rule_year_bins_host(p, s.seed, s.stream, s.begin, s.n, s.wm, _rule(c), **kw)
        except RuntimeError as e:
            refused = "code -4" in str(e) and "frozen income streams exceed the LDS budget" in str(e)
            assert refused and s.frozen_streams() > 0 and name == "default edges", (str(e), name, c.context("rule yearly bins"))
            print(f"{c.id}: {s.frozen_streams()} frozen streams: refused on the default edges ({e}); compared on the 64-bin edges")
            continue
        try:
            _check_against_rule_launch(yb, a["multipliers"], a, cnt, s.n, s.wm)
        except AssertionError as e:
            raise AssertionError(f"{e.args}: {c.context('rule yearly bins, ' + name)}") from e
        break
    # failures before retirement (bin 0) are the paths of the summary launch with YearsToRuin 0.0
    assert int(yb["ruin_year_bins"][0]) == int(np.count_nonzero(a["years_to_ruin"] == 0.0)), c.context("rule yearly bins: failures before retirement")


# ---- an exact tie is neither a cut nor a raise ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", range(len(RF.TIES)))
def test_an_exact_tie_keeps_the_multiplier(oracle, j):
    """`rule_fuzz.tie_cases`: (m r0) P == upper B == lower B every year (the plain launch's own trajectory shows it: flat to the
    bit, price level 1.0), and the rule cuts on `>` and raises on `<`: every route keeps m = 1 and counts no cut and no raise,
    as the CPU model does."""
    c = RF.tie_cases(oracle)[j]
    s, ry = c.scn, RF.TIE_YEARS
    cpu = RF.answer(oracle, c)
    plain = E.run_batch_host(c.params(), s.seed, s.stream, s.begin, s.n, s.wm, want_bins=False)
    b0 = plain["start_balance"]
    assert np.all(plain["inflation_at_retirement"] == 1.0) and np.all(plain["trajectory"][-ry:] == b0[None, :]), c.context("plain launch: not flat")
    assert np.all(plain["real_trajectory"][-ry:] == b0[None, :]) and np.array_equal(b0, np.array([float(r["start_balance"][0]) for r in cpu["runs"]]))
    want = cpu["year_counts"]
    assert want.tolist() == [[s.n, 0, 0, 0]] * ry
    got = _launch(c, want="summary", multipliers=True)
    assert np.array_equal(_bits(got["multipliers"]), _bits(cpu["rows"])), c.context("summary: rows")
    assert np.array_equal(got["year_counts"].astype(np.int64), want) and got["counters"].tolist() == [s.n, s.n], c.context("summary")
    assert np.array_equal(_launch(c)["year_counts"].astype(np.int64), want), c.context("count-only")
    amounts = (float(s.cfgd["initial_balance"]), float(s.cfgd["monthly_contribution"]), 0.0)
    counts, years = E.probe_rules(c.params(), s.seed, s.stream, s.begin, s.n, s.wm, [amounts + (_rule(c),), amounts + (_rule(c, "pinned"),)])
    assert int(N.load_library().mcr_probe_rules_last_fanout_launches()) == 1
    assert np.array_equal(years.cpu().numpy(), np.stack([want, want])) and counts.cpu().numpy().tolist() == [[s.n, s.n]] * 2, c.context("rule fan-out")
    counts, years = E.probe_rule_grid(c.params(), s.seed, s.stream, s.begin, s.n, [s.wm, s.wm + 12], [[0.0], [0.0]], _rule(c))
    assert int(N.load_library().mcr_probe_rule_grid_last_fanout_launches()) == 1
    assert np.array_equal(years.cpu().numpy()[:, 0], np.stack([want, want])), c.context("rule grid")
    yb = E.run_rule_year_bins_host(c.params(), s.seed, s.stream, s.begin, s.n, s.wm, _rule(c))
    assert np.array_equal(yb["rule_year_counts"].astype(np.int64), want), c.context("rule yearly bins")
    one = int(np.argmax(np.concatenate(([0], np.histogram([1.0], bins=yb["m_edges"])[0], [0]))))
    assert np.all(yb["multiplier_bins"][:, one] == s.n) and int(yb["multiplier_bins"].sum()) == ry * s.n, c.context("rule yearly bins: multiplier_bins")


# ---- what the rule launch refuses among count_fuzz's plans ---------------------------------------------------------------------------
def test_generic_plans_are_refused_by_name_and_compute_nothing(oracle):
    """A `generic` plan of each kind (even index: 17-20 paying income streams; odd: a rate the exact month is for)."""
    import torch

    lib = N.load_library()
    dev = torch.device("cuda", 0)
    rule = SpendingRule(*RF.RULES["symmetric"])
    for scn, word in zip(F.scenarios(oracle, "generic")[:2], ("income streams", "exact month")):
        p = scn.params()
        ry = int(scn.cfgd["retirement_years"])
        counts = torch.full((2 + 4 * ry,), SENTINEL, dtype=torch.int64, device=dev)
        success = torch.full((scn.n,), 9, dtype=torch.uint8, device=dev)
        rows = torch.full((ry, scn.n), float(SENTINEL), dtype=torch.float64, device=dev)
        o = N.McrOutputs()
        o.path_stride, o.counters, o.success = scn.n, counts.data_ptr(), success.data_ptr()
        ro = N.McrRuleOutputs()
        ro.year_counts, ro.multipliers, ro.path_stride = counts[2:].data_ptr(), rows.data_ptr(), scn.n
        rec, rng = rule.record(), N.philox_rng(scn.seed)
        rc = lib.mcr_run_rule_rng(C.byref(p), C.byref(rng), scn.stream, scn.begin, scn.n, scn.wm, C.byref(rec), C.byref(o), C.byref(ro), 0, None)
        msg = N.last_error()
        torch.cuda.synchronize()
        touched = bool((counts != SENTINEL).any() or (success != 9).any() or (rows != SENTINEL).any())
        assert rc == N.MCR_ERR_UNSUPPORTED and word in msg and not touched, (rc, msg, touched, scn.context("rule launch"))
        with pytest.raises(RuntimeError, match="code -4"):
            E.run_rule_host(p, scn.seed, scn.stream, scn.begin, scn.n, scn.wm, rule)
