"""CPU-only checks of the joint-outcome layer: `paired.JointOutcomes` against brute force, the exact McNemar p-value against
`math.comb`, the unchanged documents of `compare_claiming_options` / `stress_test` with ``paired=False``, and the new C-ABI
entries (declared, bound, and rejecting bad arguments before any device call)."""

from __future__ import annotations

import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.income import INCOME_OPTION_FIELDS
from monte_carlo_retirement_amd.paired import JointOutcomes, mcnemar_p_value
from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

JOINT_SYMBOLS = ("mcr_joint_mask_words", "mcr_probe_scenarios_joint_rng", "mcr_probe_assumptions_joint_rng",
                 "mcr_probe_income_joint_rng", "mcr_joint_counts")
DIFFERENCE_KEYS = {"delta", "se", "se_unpaired", "p_value", "rescued"}


@pytest.fixture(scope="module")
def lib():
    from monte_carlo_retirement_amd.csrc import build

    build.build()
    return N.load_library()


# ---- JointOutcomes against brute force -----------------------------------------------------------------------------------
def _flags(seed, k, n):
    """k options x n paths of 0/1 flags with a shared component, so options agree on most paths (like shared random numbers)."""
    rng = np.random.default_rng(seed)
    common = rng.random(n)
    return np.stack([(common + 0.15 * rng.standard_normal(n) < 0.35 + 0.4 * rng.random()).astype(np.int64) for _ in range(k)])


@pytest.mark.parametrize("seed,k,n", [(1, 2, 50), (2, 5, 1000), (3, 15, 4133), (4, 32, 777), (5, 1, 9)])
def test_joint_outcomes_equal_brute_force(seed, k, n):
    F = _flags(seed, k, n)
    every, none = int(F.all(axis=0).sum()), int((~F.any(axis=0)).sum())
    J = JointOutcomes(F @ F.T, n, (every, none))
    assert len(J) == k and J.n_paths == n
    assert J.successes.tolist() == F.sum(axis=1).tolist()
    assert J.probabilities.dtype == np.float64
    assert J.probabilities.tolist() == [float(np.float64(int(c)) / np.float64(n) * 100.0) for c in F.sum(axis=1)]
    assert (J.all_succeed, J.none_succeed) == (every, none)
    for a in range(k):
        for b in range(k):
            fa, fb = F[a].astype(bool), F[b].astype(bool)
            table = {"both": int((fa & fb).sum()), "only_a": int((fa & ~fb).sum()), "only_b": int((~fa & fb).sum()),
                     "neither": int((~fa & ~fb).sum())}
            assert J.pair(a, b) == table
            d = J.difference(a, b)
            assert set(d) == DIFFERENCE_KEYS
            diff = fa.astype(np.float64) - fb.astype(np.float64)       # the per-path paired difference
            assert d["delta"] == pytest.approx(100.0 * diff.mean(), abs=1e-12)
            # the standard error of the mean of `diff` (population variance / n): the paired formula restated
            assert d["se"] == pytest.approx(100.0 * math.sqrt(diff.var() / n), rel=1e-9, abs=1e-12)
            pa, pb = fa.mean(), fb.mean()
            assert d["se_unpaired"] == pytest.approx(100.0 * math.sqrt(pa * (1 - pa) / n + pb * (1 - pb) / n), rel=1e-12)
            fails = int((~fa).sum())
            assert d["rescued"] == (None if fails == 0 else table["only_b"] / fails)
            assert d["p_value"] == mcnemar_p_value(table["only_a"], table["only_b"])


def test_paired_error_is_smaller_when_options_share_paths():
    F = _flags(7, 2, 20_000)
    d = JointOutcomes(F @ F.T, F.shape[1]).difference(0, 1)
    assert 0.0 < d["se"] < d["se_unpaired"]


def test_extremes_are_optional():
    J = JointOutcomes([[3, 2], [2, 4]], 10)
    assert J.extremes is None and J.all_succeed is None and J.none_succeed is None
    with pytest.raises(ValueError):
        JointOutcomes([[1, 2, 3]], 10)


# ---- the exact McNemar p-value --------------------------------------------------------------------------------------------
def _exact(n10, n01):
    m, k = n10 + n01, min(n10, n01)
    if m == 0:
        return 1.0
    return min(1.0, 2.0 * sum(math.comb(m, i) for i in range(k + 1)) / 2.0 ** m)


def test_p_value_equals_the_exact_binomial_sum():
    for n10 in range(41):
        for n01 in range(41 - n10):
            got = mcnemar_p_value(n10, n01)
            assert got == pytest.approx(_exact(n10, n01), rel=1e-11), (n10, n01)
            assert got == mcnemar_p_value(n01, n10)              # symmetric in a <-> b
            assert 0.0 < got <= 1.0
    assert mcnemar_p_value(0, 0) == 1.0


def test_p_value_through_difference_is_symmetric_and_one_without_discordant_paths():
    J = JointOutcomes([[40, 30, 40], [30, 55, 30], [40, 30, 40]], 100)
    assert J.difference(0, 1)["p_value"] == J.difference(1, 0)["p_value"] == mcnemar_p_value(10, 25)
    assert J.difference(0, 2)["p_value"] == 1.0 and J.difference(0, 2)["delta"] == 0.0 and J.difference(0, 2)["se"] == 0.0
    assert J.difference(0, 1)["delta"] == -J.difference(1, 0)["delta"] == -15.0


def test_p_value_survives_a_million_discordant_paths():
    p = mcnemar_p_value(10**6, 0)
    assert math.isfinite(p) and 0.0 < p <= 1.0
    assert mcnemar_p_value(0, 10**6) == p
    near = mcnemar_p_value(500_500, 499_500)                     # 10^6 discordant, one standard deviation apart
    assert near == pytest.approx(math.erfc(1000.0 / math.sqrt(2.0 * 10**6)), rel=5e-3)   # the normal limit, continuity aside


def test_p_value_decreases_as_the_imbalance_grows():
    for m in (1, 2, 7, 40, 41, 500, 10_001):
        ps = [mcnemar_p_value(m - k, k) for k in range(m // 2, -1, -1)]      # k = m/2 (balanced) down to 0
        assert all(a >= b for a, b in zip(ps, ps[1:])), m
        assert ps[0] > ps[-1] or m == 1
        assert ps[0] == pytest.approx(1.0, abs=0.05) or m < 7
    assert mcnemar_p_value(1, 0) == 1.0 and mcnemar_p_value(3, 3) == 1.0
    with pytest.raises(ValueError):
        mcnemar_p_value(-1, 3)


def test_rescued_is_none_when_a_never_fails():
    J = JointOutcomes([[10, 7], [7, 7]], 10)
    assert J.difference(0, 1)["rescued"] is None
    assert J.difference(1, 0)["rescued"] == 1.0                  # b = option 0 turns every one of option 1's three failures round
    assert J.pair(1, 0) == {"both": 7, "only_a": 0, "only_b": 3, "neither": 0}


def test_indistinguishable_from():
    # option 1 differs from option 0 on 3 + 2 paths (p = 1.0), option 2 on 40 + 0 (p ~ 2e-12)
    J = JointOutcomes([[500, 497, 460], [497, 499, 458], [460, 458, 460]], 1000)
    assert J.indistinguishable_from(0) == [0, 1]
    assert J.indistinguishable_from(2) == [2]
    assert J.indistinguishable_from(0, alpha=1e-15) == [0, 1, 2]


# ---- the simulator's documents ---------------------------------------------------------------------------------------------
def _simulator():
    return RetirementMonteCarloSimulator(Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json"))))


OPTIONS = [{"start_at_age": 62.0, "monthly_amount_today": 1400.0}, {"start_at_age": 67.0, "monthly_amount_today": 2000.0},
           {"start_at_age": 70.0, "monthly_amount_today": 2480.0}]


def test_claiming_document_is_unchanged_without_paired(monkeypatch):
    sim = _simulator()
    monkeypatch.setattr(sim, "success_probability_by_income_options", lambda wm, s, o, n=None: np.array([60.0, 75.5, 75.5]))
    monkeypatch.setattr(sim, "joint_outcomes_by_income_options", lambda *a, **k: pytest.fail("paired=False must not run the joint probe"))
    for doc in (sim.compare_claiming_options(240, 0, OPTIONS, 1000), sim.compare_claiming_options(240, 0, OPTIONS, 1000, paired=False)):
        assert set(doc) == {"stream", "options", "best"}
        assert doc["best"] == 1 and doc["stream"] == 0
        assert all(set(r) == set(INCOME_OPTION_FIELDS) | {"probability"} for r in doc["options"])


def test_claiming_document_with_paired(monkeypatch):
    sim = _simulator()
    J = JointOutcomes([[600, 590, 580], [590, 755, 700], [580, 700, 755]], 1000, (570, 200))
    monkeypatch.setattr(sim, "joint_outcomes_by_income_options", lambda wm, s, o, n=None: J)
    monkeypatch.setattr(sim, "success_probability_by_income_options", lambda *a, **k: pytest.fail("one probe serves paired=True"))
    doc = sim.compare_claiming_options(240, 0, OPTIONS, 1000, paired=True)
    assert set(doc) == {"stream", "options", "best", "tied_with_best", "all_succeed", "none_succeed"}
    assert doc["best"] == 1 and (doc["all_succeed"], doc["none_succeed"]) == (570, 200)
    assert [r["probability"] for r in doc["options"]] == J.probabilities.tolist()
    assert all(set(r) == set(INCOME_OPTION_FIELDS) | {"probability", "vs_best"} for r in doc["options"])
    assert [r["vs_best"] for r in doc["options"]] == [J.difference(1, i) for i in range(3)]
    assert doc["tied_with_best"] == [1, 2]                       # 55 against 55 discordant paths: no evidence either way
    assert doc["options"][0]["vs_best"]["p_value"] < 1e-20      # 165 against 10


def test_stress_table_is_unchanged_without_paired(monkeypatch):
    sim = _simulator()
    shifts = [("equity -1", {"inv1_returns_mean": -0.01}), ("inflation +1", {"inflation_rate_mean": 0.01})]
    monkeypatch.setattr(sim, "success_probability_by_assumptions", lambda wm, s, n=None: np.array([80.0, 70.0, 78.0]))
    monkeypatch.setattr(sim, "joint_outcomes_by_assumptions", lambda *a, **k: pytest.fail("paired=False must not run the joint probe"))
    for table in (sim.stress_test(240, shifts, 1000), sim.stress_test(240, shifts, 1000, paired=False)):
        assert len(table) == 3 and all(set(r) == {"label", "overrides", "probability", "delta"} for r in table)
        assert [r["delta"] for r in table] == [0.0, -10.0, -2.0]


def test_stress_table_with_paired(monkeypatch):
    sim = _simulator()
    shifts = [("equity -1", {"inv1_returns_mean": -0.01}), ("inflation +1", {"inflation_rate_mean": 0.01})]
    J = JointOutcomes([[800, 700, 775], [700, 700, 690], [775, 690, 780]], 1000, (690, 195))
    monkeypatch.setattr(sim, "joint_outcomes_by_assumptions", lambda wm, s, n=None: J)
    table = sim.stress_test(240, shifts, 1000, paired=True)
    assert all(set(r) == {"label", "overrides", "probability", "delta", "vs_base"} for r in table)
    assert all(set(r["vs_base"]) == DIFFERENCE_KEYS | {"hurt", "helped"} for r in table)
    assert [(r["vs_base"]["hurt"], r["vs_base"]["helped"]) for r in table] == [(0, 0), (100, 0), (25, 5)]
    assert [r["vs_base"]["delta"] for r in table] == [0.0, 10.0, 2.0]      # base minus row, in points
    assert [r["delta"] for r in table] == pytest.approx([0.0, -10.0, -2.0])
    assert [r["probability"] for r in table] == J.probabilities.tolist()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_native_binds_the_joint_entries(lib):
    hdr = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert re.search(r"^#define MCR_MAX_JOINT_OPTIONS 32\b", hdr, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in JOINT_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", code), sym
        assert sym in N.ABI_SYMBOLS and hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes is not None, sym
    assert N.MCR_MAX_JOINT_OPTIONS == 32
    assert len(lib.mcr_probe_income_joint_rng.argtypes) == len(lib.mcr_probe_income_rng.argtypes) + 3
    assert len(lib.mcr_probe_scenarios_joint_rng.argtypes) == len(lib.mcr_probe_scenarios_rng.argtypes) + 3
    assert len(lib.mcr_probe_assumptions_joint_rng.argtypes) == len(lib.mcr_probe_assumptions_rng.argtypes) + 3


def test_abi_version_stays_8(lib):
    assert lib.mcr_abi_version() == 8 == N.MCR_ABI_VERSION


def test_mask_words(lib):
    for n, w in ((0, 0), (1, 1), (63, 1), (64, 1), (65, 2), (4133, 65), (64_000, 1000), (2**40 + 1, 2**34 + 1), (2**64 - 1, 2**58)):
        assert lib.mcr_joint_mask_words(n) == w, n


def test_invalid_joint_arguments_return_before_any_device_call(lib):
    """The option cap and the null matrix are checked first: the answer is MCR_ERR_INVALID_ARG (-1) with or without a GPU,
    never MCR_ERR_NO_DEVICE, and no pointer is touched (they are small integers here)."""
    p = params_from_config(Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json"))))
    rng = N.McrRng()
    rng.kind, rng.philox_seed = N.MCR_RNG_PHILOX, 1
    head = (C.byref(p), C.byref(rng), 0, 0, 1000, 12)
    fake = C.c_void_p(8)
    sc = (N.McrScenario * 33)()
    am = (N.McrAssumptions * 33)()
    io = (N.McrIncomeOption * 33)()
    calls = {
        "scenarios": lambda n, joint: lib.mcr_probe_scenarios_joint_rng(*head, sc, n, fake, None, joint, None, 0, None),
        "assumptions": lambda n, joint: lib.mcr_probe_assumptions_joint_rng(*head, am, n, fake, None, joint, None, 0, None),
        "income": lambda n, joint: lib.mcr_probe_income_joint_rng(*head, 0, io, n, fake, None, joint, None, 0, None),
        "counts": lambda n, joint: lib.mcr_joint_counts(fake, n, 1000, joint, None, 0, None),
    }
    for name, call in calls.items():
        for n in (33, 1000, -1):
            assert call(n, fake) == -1, (name, n)
            assert "MCR_MAX_JOINT_OPTIONS = 32" in N.last_error(), (name, n, N.last_error())
        assert call(3, None) == -1 and "joint" in N.last_error(), name
    assert lib.mcr_joint_counts(fake, 0, 1000, None, None, 0, None) == 0      # no options: nothing touched
