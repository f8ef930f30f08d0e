"""CPU checks of the history stream (rng="history"; include/mcr.h: MCR_RNG_HISTORY): the CPU restatement the GPU tests compare
with is held to the oracle's Philox, `MarketHistory` inverts the month's growth formula, every validation error names its
field, and the library judges a history descriptor before it looks for a device."""

from __future__ import annotations

import json
import math
import os

import numpy as np
import pytest

import history_fuzz as HF
from conftest import REPO
from monte_carlo_retirement_amd import Config, MarketHistory, load_config_from_json, params_from_config, with_fitted_market
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.history import market_document
from test_abi_cpu import _child


def _record(n=240, seed=7):
    """Simple monthly returns of three series with fat tails: equity, inflation, the second asset's nominal return."""
    rng = np.random.default_rng(seed)
    eq = np.expm1(0.006 + 0.045 * rng.standard_t(5, n) / math.sqrt(5 / 3))
    inf = np.expm1(0.0025 + 0.004 * rng.standard_normal(n))
    prem = np.expm1(0.001 + 0.01 * rng.standard_normal(n))
    return eq, inf, (1 + inf) * (1 + prem) - 1, prem


def test_helper_philox_equals_the_oracles(oracle):
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 2 ** 32, size=(200, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=2, dtype=np.uint64)
    ctr[:5, 1] = (0, 1, 2 ** 32 - 1, 7, 255)          # path_hi words: paths at and above 2^32
    ctr[5:8, :] = ((0, 0, 0, 0), (2 ** 32 - 1,) * 4, (1, 0, 0, 1))
    got = np.stack(HF.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[0], key[1]), axis=1)
    want = np.array([oracle.philox4x32_10([int(x) for x in c], [int(k) for k in key]) for c in ctr], dtype=np.uint64)
    assert np.array_equal(got, want)


def test_history_rows_follow_the_rule_word_by_word(oracle):
    """`history_rows` against the header's rule spelt out with Python integers and the oracle's Philox, path >= 2^32 included."""
    seed, stream, H, B = 2 ** 40 + 12345, 1, 13, 5
    for begin in (0, 2 ** 32 - 3):
        rows = HF.history_rows(seed, stream, begin, 6, 4 * B + 1, H, B)
        for i in range(6):
            path = begin + i
            for r in range(4 * B + 1):
                k, j = divmod(r, B)
                x = oracle.philox4x32_10([path & 0xFFFFFFFF, path >> 32, k >> 2, stream], [seed & 0xFFFFFFFF, seed >> 32])[k & 3]
                assert rows[i, r] == (((x * H) >> 32) + j) % H, (begin, i, r)
    assert np.array_equal(HF.history_rows(3, 0, 0, 4, 9, 1, 2), np.zeros((4, 9), dtype=np.int64))       # one month: always it
    one = HF.history_rows(3, 0, 0, 4, 30, 7, 1000)                                                       # one block: the record run forward
    assert np.array_equal(one, (one[:, :1] + np.arange(30)[None, :]) % 7)


def test_synthetic_record_is_standardised_and_reproducible():
    z = HF.synthetic_record()
    assert z.shape == (600, 3) and np.all(np.isfinite(z))
    np.testing.assert_allclose(z.mean(axis=0), 0.0, atol=1e-12)
    np.testing.assert_allclose(z.std(axis=0), 1.0, rtol=1e-12)
    assert np.corrcoef(z[:, 0], z[:, 1])[0, 1] > 0.15          # the 0.3 mix shows
    assert np.abs(z).max() > 4.0                               # t(5) tails: a normal sample of 1 800 has none (p < 0.12)
    h = MarketHistory(z)
    assert h.months == 600 and h.block_months == 12 and h.fitted is None and not h.z.flags.writeable


def test_from_monthly_returns_inverts_the_growth_formula(oracle):
    """oracle.monthly_gross(mu_log, sigma_log, z) gives every input gross return back.  ln g carries a few ulps of error
    (2e-16 relative to |ln g| <= 0.3, i.e. ~1e-16 on g); 1e-12 leaves four decades."""
    eq, inf, inv2, prem = _record()
    h = MarketHistory.from_monthly_returns(eq, inf, inv2=inv2, block_months=6)
    assert h.months == 240 and h.block_months == 6
    want = np.stack([1 + eq, 1 + inf, (1 + inv2) / (1 + inf)], axis=1)
    for c, key in enumerate(("inv1", "inflation", "inv2_premium")):
        mu, sigma = h.fitted[key]
        got = np.array([oracle.monthly_gross(mu, sigma, float(z)) for z in h.z[:, c]])
        np.testing.assert_allclose(got, want[:, c], rtol=1e-12, atol=0.0, err_msg=key)
        np.testing.assert_allclose([h.z[:, c].mean(), h.z[:, c].std()], [0.0, 1.0], atol=1e-12)
    # the premium given directly is the same record
    g = MarketHistory.from_monthly_returns(eq, inf, premium=prem)
    np.testing.assert_allclose(g.z, h.z, rtol=0, atol=1e-9)
    for key in ("inv1", "inflation", "inv2_premium"):
        np.testing.assert_allclose(g.fitted[key], h.fitted[key], rtol=1e-9, atol=1e-12)
    assert g.fitted["equity_inflation_correlation"] == pytest.approx(float(np.corrcoef(np.log1p(eq), np.log1p(inf))[0, 1]), abs=1e-12)


def test_constant_series_has_zero_shocks_and_zero_volatility(oracle):
    eq, inf, _, _ = _record(36)
    flat = np.full(36, 0.002)
    h = MarketHistory.from_monthly_returns(eq, flat, premium=np.zeros(36))
    assert np.all(h.z[:, 1] == 0.0) and np.all(h.z[:, 2] == 0.0)
    assert h.fitted["inflation"] == (12.0 * math.log(1.002), 0.0) and h.fitted["inv2_premium"] == (0.0, 0.0)
    assert oracle.monthly_gross(*h.fitted["inflation"], 0.0) == pytest.approx(1.002, rel=1e-15)
    a = h.fitted_assumptions()
    assert a["inflation_rate_volatility"] == 0.0 and a["inv2_premium_over_inflation_volatility"] == 0.0
    assert a["inv2_premium_over_inflation_mean"] == 0.0 and a["equity_inflation_correlation"] == 0.0
    one = MarketHistory.from_monthly_returns([0.01], [0.002], inv2=[0.004])       # a one-month record
    assert one.months == 1 and np.all(one.z == 0.0)


def test_from_csv_reads_named_columns(tmp_path):
    eq, inf, inv2, prem = _record(48)
    path = tmp_path / "record.csv"
    with open(path, "w") as fh:
        fh.write("month,stocks,cpi,bonds,over\n")
        for t in range(48):
            fh.write(f"{t},{float(eq[t])!r},{float(inf[t])!r},{float(inv2[t])!r},{float(prem[t])!r}\n")
    want = MarketHistory.from_monthly_returns(eq, inf, inv2=inv2, block_months=24)
    got = MarketHistory.from_csv(str(path), equity="stocks", inflation="cpi", inv2="bonds", block_months=24)
    assert np.array_equal(got.z, want.z) and got.fitted == want.fitted and got.block_months == 24
    over = MarketHistory.from_csv(str(path), equity="stocks", inflation="cpi", inv2=None, premium="over")
    assert np.array_equal(over.z, MarketHistory.from_monthly_returns(eq, inf, premium=prem).z)
    with pytest.raises(ValueError, match="equity.*no column 'equity'"):
        MarketHistory.from_csv(str(path))
    with open(path, "a") as fh:
        fh.write("48,0.01,n/a,0.0,0.0\n")
    with pytest.raises(ValueError, match="inflation.*line 50.*'n/a'"):
        MarketHistory.from_csv(str(path), equity="stocks", inflation="cpi", inv2="bonds")


def test_fitted_assumptions_map_back_through_params_from_config():
    """arithmetic -> log of the fitted arithmetic values is the fitted log pair.  Both directions lose ~1e-16 absolute on
    sigma_log^2, i.e. 1e-16 / sigma_log on sigma_log: below 1e-12 absolute for every series here (sigma_log >= 1e-2)."""
    eq, inf, inv2, _ = _record()
    h = MarketHistory.from_monthly_returns(eq, inf, inv2=inv2)
    cfg = Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json")))
    fit = with_fitted_market(cfg, h)
    assert fit is not cfg and fit.monthly_expenses == cfg.monthly_expenses and fit.other_income_streams == cfg.other_income_streams
    assert fit.equity_inflation_correlation == h.fitted["equity_inflation_correlation"]
    p = params_from_config(fit)
    got = {"inv1": (p.inv1_mu_log, p.inv1_sigma_log), "inflation": (p.inf_mu_log, p.inf_sigma_log), "inv2_premium": (p.prem_mu_log, p.prem_sigma_log)}
    for key, pair in got.items():
        assert min(h.fitted[key][1], pair[1]) >= 1e-2, key
        np.testing.assert_allclose(pair, h.fitted[key], rtol=0, atol=1e-12, err_msg=key)
    doc = market_document(h, True)
    assert doc["months"] == 240 and doc["block_months"] == 12 and doc["as_recorded"] is True and doc["fitted"] == h.fitted_assumptions()
    assert "fitted" not in market_document(MarketHistory(h.z), False)
    with pytest.raises(ValueError, match="fitted"):
        MarketHistory(h.z).fitted_assumptions()


def test_every_validation_error_names_its_field():
    z = HF.synthetic_record()
    eq, inf, inv2, prem = _record(24)
    bad = z.copy()
    bad[5, 1] = np.nan
    cases = [
        (lambda: MarketHistory(bad), "z"),
        (lambda: MarketHistory(np.where(np.arange(600)[:, None] == 3, np.inf, z)), "z"),
        (lambda: MarketHistory(z[:, :2]), "z"),
        (lambda: MarketHistory(z.reshape(-1)), "z"),
        (lambda: MarketHistory(np.zeros((0, 3))), "z"),
        (lambda: MarketHistory(np.zeros((2049, 3))), "z"),
        (lambda: MarketHistory(z, block_months=0), "block_months"),
        (lambda: MarketHistory(z, block_months=2 ** 31), "block_months"),
        (lambda: MarketHistory(z, block_months=1.5), "block_months"),
        (lambda: MarketHistory.from_monthly_returns(np.append(eq[:-1], np.nan), inf, inv2=inv2), "equity"),
        (lambda: MarketHistory.from_monthly_returns(eq, np.append(inf[:-1], -1.0), inv2=inv2), "inflation"),
        (lambda: MarketHistory.from_monthly_returns(eq, inf, inv2=np.append(inv2[:-1], -1.5)), "inv2"),
        (lambda: MarketHistory.from_monthly_returns(eq, inf, premium=np.append(prem[:-1], np.inf)), "premium"),
        (lambda: MarketHistory.from_monthly_returns(eq, inf[:-1], inv2=inv2), "inflation"),
        (lambda: MarketHistory.from_monthly_returns(eq.reshape(2, 12), inf, inv2=inv2), "equity"),
        (lambda: MarketHistory.from_monthly_returns(np.zeros(2049), np.zeros(2049), inv2=np.zeros(2049)), "equity"),
        (lambda: MarketHistory.from_monthly_returns(eq, inf), "inv2 / premium"),
        (lambda: MarketHistory.from_monthly_returns(eq, inf, inv2=inv2, premium=prem), "inv2 / premium"),
        (lambda: MarketHistory.from_monthly_returns(eq, inf, inv2=inv2, block_months=-1), "block_months"),
        (lambda: N.history_rng(1, bad, 12), "history table"),
        (lambda: N.history_rng(1, z[:, :2], 12), "history table"),
        (lambda: N.history_rng(1, np.zeros((2049, 3)), 12), "history table"),
        (lambda: N.history_rng(1, z, 0), "history block"),
    ]
    for make, field in cases:
        with pytest.raises(ValueError, match=field):
            make()
    MarketHistory(np.zeros((2048, 3)), block_months=2 ** 31 - 1)      # the limits themselves are fine
    MarketHistory(np.zeros((1, 3)), block_months=1)


def test_simulator_takes_a_history_only_with_rng_history():
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    cfg = Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json")))
    h = MarketHistory(HF.synthetic_record(), block_months=12)
    with pytest.raises(ValueError, match="market_history"):
        RetirementMonteCarloSimulator(cfg, main_seed_override=1, rng="history")
    with pytest.raises(ValueError, match="market_history"):
        RetirementMonteCarloSimulator(cfg, main_seed_override=1, rng="philox", market_history=h)
    with pytest.raises(ValueError, match="market_history"):
        RetirementMonteCarloSimulator(cfg, main_seed_override=1, rng="numpy", market_history=h)
    with pytest.raises(ValueError, match="MarketHistory"):
        RetirementMonteCarloSimulator(cfg, main_seed_override=1, rng="history", market_history=h.z)
    with pytest.raises(ValueError, match="rng must be"):
        RetirementMonteCarloSimulator(cfg, main_seed_override=1, rng="record")
    sim = RetirementMonteCarloSimulator(cfg, main_seed_override=2 ** 70 + 5, rng="history", market_history=h)
    r = sim._batch_rng(1000)
    assert r.kind == N.MCR_RNG_HISTORY and r.history_months == 600 and r.history_block == 12 and r.philox_seed == sim._engine_seed
    assert r.history == r._history_table.ctypes.data and np.array_equal(r._history_table, h.z)
    assert sim._path_seeds(5) == [0, 1, 2, 3, 4]


def test_descriptor_layout_and_header():
    r = N.McrRng()
    assert r.kind == N.MCR_RNG_PHILOX and r.history is None and r.history_months == 0 and r.history_block == 0
    assert N.McrRng.history.offset == N.McrRng.path_seeds.offset + 8 and N.McrRng.history_block.offset == N.McrRng.history_months.offset + 4
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert "#define MCR_RNG_HISTORY 2u" in header and f"#define MCR_MAX_HISTORY_MONTHS {N.MCR_MAX_HISTORY_MONTHS}" in header
    assert "#define MCR_ABI_VERSION 8" in header and N.MCR_RNG_HISTORY == 2


def test_library_judges_a_history_descriptor_before_the_device():
    """mcr_run_batch_host_rng, in a child process (a HIP runtime initialised here would stay open for the session): a bad
    history descriptor is MCR_ERR_INVALID_ARG with the field in the message, with or without a GPU; a good one then fails for
    want of a device where there is none (or runs)."""
    code = r"""
import ctypes as C, json, numpy as np
from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config
from monte_carlo_retirement_amd import _native as N
lib = N.load_library()
p = params_from_config(Config(**load_config_from_json("scenarios/config.json")))
z = np.zeros((2049, 3))
nan = np.zeros((4, 3)); nan[2, 1] = np.nan
def call(table, months, block):
    r = N.McrRng(); r.kind = N.MCR_RNG_HISTORY; r.philox_seed = 1
    r.history = table.ctypes.data if table is not None else None
    r.history_months = months; r.history_block = block
    counters = np.zeros(2, dtype=np.uint64)
    o = N.McrOutputs(); o.counters = counters.ctypes.data
    rc = lib.mcr_run_batch_host_rng(C.byref(p), C.byref(r), 1, 0, 8, 12, None, C.byref(o), 0)
    return [int(rc), N.last_error(), int(counters[1])]
out = {"gpu": int(lib.mcr_device_count()) > 0,
       "H0": call(z, 0, 12), "B0": call(z, 600, 0), "H2049": call(z, 2049, 12), "Bbig": call(z, 600, 2 ** 31),
       "null": call(None, 600, 12), "nan": call(nan, 4, 12), "ok": call(z, 600, 12)}
r = N.McrRng(); r.kind = 3
o = N.McrOutputs()
out["kind3"] = [int(lib.mcr_run_batch_host_rng(C.byref(p), C.byref(r), 1, 0, 8, 12, None, C.byref(o), 0)), N.last_error(), 0]
print(json.dumps(out))
"""
    out = json.loads(_child(code).strip().splitlines()[-1])
    for key, field in (("H0", "history_months = 0"), ("B0", "history_block = 0"), ("H2049", "history_months = 2049"),
                       ("Bbig", "history_block = 2147483648"), ("null", "null history table"), ("nan", r"history[2][1]")):
        rc, msg, paths = out[key]
        assert rc == -1 and field in msg and "history rng" in msg and paths == 0, (key, out[key])
    rc, msg, paths = out["ok"]
    if out["gpu"]:
        assert rc == 0 and paths == 8, out["ok"]
        assert out["kind3"][0] == -1 and "unknown rng kind 3" in out["kind3"][1]
    else:
        assert rc == -2 and "no usable HIP device" in msg, out["ok"]
        assert out["kind3"][0] == -2      # (the other kinds keep their order: the device first)
