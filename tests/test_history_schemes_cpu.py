"""CPU checks of the history stream's schemes (include/mcr.h: MCR_HISTORY_BLOCK / _STATIONARY / _COHORTS): the Python surface
takes and names them, the descriptor carries them behind the fields it had, the library judges them before it looks for a
device, `CohortReplay` does its arithmetic, and the CPU restatement the GPU tests compare with behaves like a stationary
bootstrap."""

from __future__ import annotations

import json
import math
import os

import numpy as np
import pytest

import history_fuzz as HF
import history_scheme_fuzz as SF
from conftest import REPO
from monte_carlo_retirement_amd import Config, MarketHistory, load_config_from_json
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.cohorts import CohortReplay
from monte_carlo_retirement_amd.history import market_document
from test_abi_cpu import _child


def _returns(n=48, seed=11):
    rng = np.random.default_rng(seed)
    return tuple(np.expm1(m + s * rng.standard_normal(n)) for m, s in ((0.006, 0.04), (0.003, 0.004), (0.002, 0.01)))


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
def test_market_history_takes_three_schemes_and_a_first_month():
    z = HF.synthetic_record()
    assert MarketHistory(z).scheme == "block" and MarketHistory(z).first_month is None
    for scheme in ("block", "stationary", "cohorts"):
        h = MarketHistory(z, 6, scheme=scheme, first_month="1926-01")
        assert h.scheme == scheme and h.first_month == "1926-01" and h.block_months == 6
    for bad in ("fixed", "", None, 1, "Block"):
        with pytest.raises(ValueError, match="scheme"):
            MarketHistory(z, scheme=bad)
    for bad in ("1926", "1926-13", "1926-00", "26-01", "1926-1", 192601, "1926-01-01"):
        with pytest.raises(ValueError, match="first_month"):
            MarketHistory(z, first_month=bad)
    with pytest.raises(TypeError):
        MarketHistory(z, 12, None, "stationary")          # keyword-only: the positional arguments are the ones it had


def test_constructors_pass_the_scheme_and_the_first_month_on(tmp_path):
    eq, inf, prem = _returns()
    h = MarketHistory.from_monthly_returns(eq, inf, premium=prem, block_months=7, scheme="stationary", first_month="1871-02")
    assert (h.scheme, h.first_month, h.block_months) == ("stationary", "1871-02", 7)
    assert MarketHistory.from_monthly_returns(eq, inf, premium=prem).scheme == "block"
    path = tmp_path / "record.csv"
    with open(path, "w") as fh:
        fh.write("equity,inflation,premium\n")
        for t in range(len(eq)):
            fh.write(f"{float(eq[t])!r},{float(inf[t])!r},{float(prem[t])!r}\n")
    c = MarketHistory.from_csv(str(path), inv2=None, premium="premium", scheme="cohorts", first_month="1999-12")
    assert (c.scheme, c.first_month) == ("cohorts", "1999-12") and np.array_equal(c.z, MarketHistory.from_monthly_returns(eq, inf, premium=prem).z)
    with pytest.raises(ValueError, match="scheme"):
        MarketHistory.from_csv(str(path), inv2=None, premium="premium", scheme="replay")
    with pytest.raises(ValueError, match="first_month"):
        MarketHistory.from_monthly_returns(eq, inf, premium=prem, first_month="Jan 1926")


def test_market_document_is_unchanged_for_blocks_and_names_the_other_schemes():
    eq, inf, prem = _returns()
    h = MarketHistory.from_monthly_returns(eq, inf, premium=prem, block_months=6)
    assert market_document(h, True) == {"months": 48, "block_months": 6, "as_recorded": True, "fitted": h.fitted_assumptions()}
    assert market_document(MarketHistory(h.z), False) == {"months": 48, "block_months": 12, "as_recorded": False}
    s = MarketHistory(h.z, 9, scheme="stationary")
    assert market_document(s, False) == {"months": 48, "block_months": 9, "as_recorded": False, "scheme": "stationary"}
    c = MarketHistory(h.z, scheme="cohorts", first_month="1926-01")
    assert market_document(c, False) == {"months": 48, "block_months": 12, "as_recorded": False, "scheme": "cohorts", "first_month": "1926-01"}
    assert market_document(MarketHistory(h.z, first_month="1926-01"), False) == {"months": 48, "block_months": 12, "as_recorded": False,
                                                                                 "first_month": "1926-01"}
    json.dumps(market_document(c, False))


def test_simulator_passes_the_scheme_into_its_descriptor_and_guards_the_cohort_replay():
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json")))
    z = HF.synthetic_record()
    for scheme, code in (("block", 0), ("stationary", 1), ("cohorts", 2)):
        sim = RetirementMonteCarloSimulator(cfg, main_seed_override=5, rng="history", market_history=MarketHistory(z, 12, scheme=scheme))
        r = sim._batch_rng(1000)
        assert r.kind == N.MCR_RNG_HISTORY and r.history_scheme == code and r.history_reserved == 0 and r.history_block == 12
        if scheme != "cohorts":
            with pytest.raises(ValueError, match="cohorts"):
                sim.historical_cohorts(233)
    with pytest.raises(ValueError, match="cohorts"):
        RetirementMonteCarloSimulator(cfg, main_seed_override=5).historical_cohorts(233)


# ---- the descriptor -------------------------------------------------------------------------------------------------------------
def test_descriptor_carries_the_scheme_behind_the_block_length():
    r = N.McrRng()
    assert r.history_scheme == 0 and r.history_reserved == 0
    assert N.McrRng.history_scheme.offset == N.McrRng.history_block.offset + 4 and N.McrRng.history_reserved.offset == N.McrRng.history_scheme.offset + 4
    assert N.McrRng.history_block.offset == N.McrRng.history_months.offset + 4 and N.McrRng.history.offset == N.McrRng.path_seeds.offset + 8
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    for name, value in (("MCR_HISTORY_BLOCK", 0), ("MCR_HISTORY_STATIONARY", 1), ("MCR_HISTORY_COHORTS", 2)):
        assert any(line.split()[:3] == ["#define", name, f"{value}u"] for line in header.splitlines()), name
        assert getattr(N, name) == value
    assert "uint32_t history_scheme;" in header and "uint32_t history_reserved;" in header and "#define MCR_ABI_VERSION 8" in header
    z = HF.synthetic_record()
    assert N.history_rng(1, z, 12).history_scheme == 0 and N.history_rng(1, z, 12, 1).history_scheme == 1
    assert N.history_rng(1, z, 12, scheme=2).history_scheme == 2
    for bad in (3, -1, "stationary", True):
        with pytest.raises(ValueError, match="history scheme"):
            N.history_rng(1, z, 12, bad)


def test_library_judges_the_scheme_before_the_device():
    """mcr_run_batch_host_rng in a child process (tests/test_history_cpu.py: why a child): an unknown scheme or a nonzero
    reserved word is MCR_ERR_INVALID_ARG with the field in the message, with or without a GPU; schemes 1 and 2 pass the check
    (and then run, or fail for want of a device)."""
    code = r"""
import ctypes as C, json, numpy as np
from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config
from monte_carlo_retirement_amd import _native as N
lib = N.load_library()
p = params_from_config(Config(**load_config_from_json("scenarios/config.json")))
z = np.zeros((600, 3))
def call(scheme, reserved):
    r = N.McrRng(); r.kind = N.MCR_RNG_HISTORY; r.philox_seed = 1
    r.history = z.ctypes.data; r.history_months = 600; r.history_block = 12
    r.history_scheme = scheme; r.history_reserved = reserved
    counters = np.zeros(2, dtype=np.uint64)
    o = N.McrOutputs(); o.counters = counters.ctypes.data
    rc = lib.mcr_run_batch_host_rng(C.byref(p), C.byref(r), 1, 0, 8, 12, None, C.byref(o), 0)
    return [int(rc), N.last_error(), int(counters[1])]
print(json.dumps({"gpu": int(lib.mcr_device_count()) > 0, "scheme3": call(3, 0), "reserved1": call(0, 1), "reserved_s1": call(1, 7),
                  "s0": call(0, 0), "s1": call(1, 0), "s2": call(2, 0)}))
"""
    out = json.loads(_child(code).strip().splitlines()[-1])
    for key, field in (("scheme3", "history_scheme = 3"), ("reserved1", "history_reserved = 1"), ("reserved_s1", "history_reserved = 7")):
        rc, msg, paths = out[key]
        assert rc == -1 and field in msg and "history rng" in msg and paths == 0, (key, out[key])
    for key in ("s0", "s1", "s2"):
        rc, msg, paths = out[key]
        if out["gpu"]:
            assert rc == 0 and paths == 8, (key, out[key])
        else:
            assert rc == -2 and "no usable HIP device" in msg, (key, out[key])


# ---- CohortReplay ---------------------------------------------------------------------------------------------------------------
def test_cohort_replay_arithmetic():
    nan = float("nan")
    #          start  0      1      2      3      4      5
    success = [True, False, True, False, True, False]
    final = [500.0, 0.0, 100.0, 0.0, 100.0, 0.0]
    ruin = [nan, 12.5, nan, 3.25, nan, 3.25]
    c = CohortReplay(success, final, ruin, total_months=4, first_month="1999-11")
    assert len(c) == 6 and c.start_row.tolist() == [0, 1, 2, 3, 4, 5]
    assert c.wraps.tolist() == [False, False, False, True, True, True]          # start + 4 > 6
    assert c.start_month == ["1999-11", "1999-12", "2000-01", "2000-02", "2000-03", "2000-04"]
    assert c.success_probability == 50.0
    assert c.success_probability_complete == float(np.float64(2) / np.float64(3) * 100.0)
    assert c.worst(6) == [3, 5, 1, 2, 4, 0]      # failures by ruin time (ties by start), then successes by what is left
    assert c.worst(2) == [3, 5] and c.worst(0) == [] and c.worst(99) == [3, 5, 1, 2, 4, 0]
    doc = c.to_document(worst=3)
    assert json.loads(json.dumps(doc)) == doc
    assert [w["start_row"] for w in doc["worst"]] == [3, 5, 1] and doc["worst"][0] == {
        "start_row": 3, "start_month": "2000-02", "wraps": True, "success": False, "final_balance": 0.0, "years_to_ruin": 3.25}
    assert doc["cohorts"] == 6 and doc["complete_cohorts"] == 3 and doc["success_probability"] == 50.0 and doc["years_to_ruin"][0] is None
    assert doc["success"] == success and doc["wraps"] == c.wraps.tolist() and doc["start_month"] == c.start_month

    every = CohortReplay(success, final, ruin, total_months=7)                     # longer than the record: every cohort wraps
    assert every.wraps.all() and every.success_probability_complete is None and every.success_probability == 50.0
    assert every.start_month == [None] * 6 and every.to_document()["start_month"] is None and every.to_document()["success_probability_complete"] is None
    edge = CohortReplay(success, final, ruin, total_months=6)                      # exactly the record: only start 0 fits
    assert edge.wraps.tolist() == [False, True, True, True, True, True] and edge.success_probability_complete == 100.0
    with pytest.raises(ValueError, match="final_balance"):
        CohortReplay(success, final[:-1], ruin, 4)


# ---- the restatement's own sanity -----------------------------------------------------------------------------------------------
def test_stationary_rows_follow_the_recipe_word_by_word(oracle):
    """`stationary_rows` against the header's recipe walked with Python integers and the oracle's Philox, paths >= 2^32 included."""
    seed, stream, H = 2 ** 40 + 12345, 1, 13
    for B in (1, 3, 5):
        for begin in (0, 2 ** 32 - 3):
            rows = SF.stationary_rows(seed, stream, begin, 6, 41, H, B)
            for i in range(6):
                path, cur = begin + i, None
                for r in range(41):
                    w = oracle.philox4x32_10([path & 0xFFFFFFFF, path >> 32, r >> 1, stream], [seed & 0xFFFFFFFF, seed >> 32])
                    a = 2 * (r & 1)
                    cur = (w[a + 1] * H) >> 32 if r == 0 or (w[a] * B) >> 32 == 0 else (cur + 1) % H
                    assert rows[i, r] == cur, (B, begin, i, r)


def test_stationary_restatement_restarts_like_a_geometric_law():
    """B = 12 on 2 000 paths x 833 rows: the restart share over rows 1 .. 832 is a binomial sample of p = 1 / 12 (the recipe's
    ceil(2^32 / 12) / 2^32 is 2e-10 above it); four standard errors.  A restart lands anywhere, a continued row is its
    predecessor + 1 mod H."""
    n, rows_n, H, B = 2000, 833, 600, 12
    rows, restart = SF.stationary_rows(2 ** 40 + 77, 1, 0, n, rows_n, H, B, restarts=True)
    assert restart[:, 0].all() and rows.min() >= 0 and rows.max() < H
    share = float(restart[:, 1:].mean())
    p = 1.0 / B
    se = math.sqrt(p * (1.0 - p) / (n * (rows_n - 1)))
    print(f"restart share excluding row 0: {share:.5f} (1 / 12 = {1 / 12:.5f}, standard error {se:.6f})")
    assert abs(share - p) <= 4.0 * se, (share, p, se)
    cont = ~restart[:, 1:]
    assert np.array_equal(rows[:, 1:][cont], ((rows[:, :-1] + 1) % H)[cont])
    assert len(np.unique(rows[:, 0])) > H // 2                                    # the starts spread over the record


def test_stationary_restatement_at_the_ends():
    rows, restart = SF.stationary_rows(3, 0, 2 ** 32 - 3, 6, 40, 13, 1, restarts=True)
    assert restart.all()                                                          # B = 1: every month a new start
    assert np.array_equal(SF.stationary_rows(3, 0, 0, 5, 9, 1, 5), np.zeros((5, 9), dtype=np.int64))      # H = 1: row 0 only
    one, restart = SF.stationary_rows(3, 0, 0, 50, 833, 7, 2 ** 31 - 1, restarts=True)
    assert not restart[:, 1:].any() and np.array_equal(one, (one[:, :1] + np.arange(833)[None, :]) % 7)  # (p = 2 / 2^32 a row)
    # a path's rows do not depend on the batch it is drawn in
    whole = SF.stationary_rows(9, 1, 2 ** 40, 20, 31, 600, 5)
    assert np.array_equal(whole[7:12], SF.stationary_rows(9, 1, 2 ** 40 + 7, 5, 31, 600, 5))


def test_cohort_restatement():
    rows = SF.cohort_rows(2 ** 40 + 5, 30, 50, 13)
    assert rows[:, 0].tolist() == [(2 ** 40 + 5 + i) % 13 for i in range(30)]
    assert np.array_equal(rows[13:26], rows[:13]) and np.array_equal(np.diff(rows, axis=1) % 13, np.ones((30, 49), dtype=np.int64))
    assert np.array_equal(SF.cohort_rows(0, 4, 5, 1), np.zeros((4, 5), dtype=np.int64))
