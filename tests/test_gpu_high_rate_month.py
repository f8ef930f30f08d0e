"""The month at realized-gains rates near 100 % (the band just below and above DevParams::exact_month, derive_params).

The path kernel runs the month in CLOSED FORM (csrc/mcr_device.h, TOLERANCE FORM) for every parameter block whose
effective realized-gains rates are <= 1 - 1e-6; above that it runs the reference's exact forms.  Two things grow as the
rate goes to 1 and are checked here against the oracle (the reference's arithmetic, bit for bit):
* amplification: cap_i = b_i - r_i G_i cancels when the gain fraction and the rate are both near 1; the reference's
  t_i / (1 - gf r) is as ill-conditioned but rounds differently — the gap grows like 2^-53 / (1 - gf r);
* the DUST sub-case: total balance > 1e-6 but total liquidation value <= 1e-6; the reference then splits the target by the
  allocation weights (simulation.py:750-755), not by capacity shares.  The kernel routes those lanes through the exact forms.
Measured on the MI355X (LABNOTES): worst path error 3.7e-12 of the path's scale over the ladder, no flag flips.

MCR_HIGH_RATE_SEED / MCR_HIGH_RATE_PATHS: longer soaks with other seeds and more paths (by hand on the GPU box; the defaults
are the suite's)."""

from __future__ import annotations

import os

import numpy as np
import pytest

from conftest import load_golden
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E

pytestmark = pytest.mark.gpu

EPS = 1e-6                          # the reference's SMALL_EPSILON dollars
U = 2.0 ** -53
REL, ABS = 1e-9, 1e-6               # the path contract (test_gpu_differential.py)
RATES = [0.99, 0.999, 0.9999, 1 - 1e-5, 1 - 2e-6, float(np.nextafter(1 - 1e-6, 0.0)), 1 - 1e-6,
         float(np.nextafter(1 - 1e-6, 1.0)), 1 - 1e-7, 1.0]
SEED = int(os.environ.get("MCR_HIGH_RATE_SEED", "20261015"))
N_PATHS = int(os.environ.get("MCR_HIGH_RATE_PATHS", "20000"))
KNOBS = ("MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS", "MCR_K1_SEGMENT_ORDER")


def _helper_cfg(rate, mask, alloc):
    base = load_golden("helpers.json")["tax_cfgs"][0]
    return dict(base, allocation_inv1_pct=alloc,
                inv1_realized_gains_tax_rate=rate if mask & 1 else 0.3, inv1_use_realized_gains_tax_system=bool(mask & 1),
                inv2_realized_gains_tax_rate=rate if mask & 2 else 0.3, inv2_use_realized_gains_tax_system=bool(mask & 2))


def _states(rng, n, rate):
    """Gains-heavy states (cost basis 0 or 1e-3 b): balances from 1e-6 to 1e14, a quarter of them in the dust band
    (1e-6, 1e-6 / (1 - r)] of the total, needs at, below and above the capacity."""
    def money(k):
        x = 10.0 ** rng.uniform(-6, 14, k)
        x = np.where(rng.integers(0, 8, k) == 0, 0.0, x)
        return x
    b1, b2 = money(n), money(n)
    top = EPS / max(1.0 - rate, 1e-7)
    dust = rng.integers(0, 4, n) == 0
    tot = rng.uniform(EPS, top, n)
    w = rng.choice([0.0, 0.5, 0.999, 1.0, rng.uniform(0, 1)], n)
    b1 = np.where(dust, tot * w, b1)
    b2 = np.where(dust, tot * (1.0 - w), b2)
    basis = lambda b: b * rng.choice([0.0, 1e-3, 1e-3 * rng.uniform(0, 1)], n)  # noqa: E731
    return b1, basis(b1), b2, basis(b2), dust


def _cap_ref(oracle, b, c, use, r):
    return np.array([oracle.nlv(b[i], c[i], use, r) for i in range(len(b))])


@pytest.mark.parametrize("rate", RATES)
def test_month_helpers_at_high_rates_are_within_their_conditioning(oracle, rate):
    """MCR_HELPER_WITHDRAW_MONTH / MCR_HELPER_REBALANCE_MONTH (the month as the kernel runs it for the block) vs the oracle's
    sequence (simulation.py:726-796), as in test_gpu_path_forms.py:  |got - exp| <= 16 u scale / max(1e-6, 1 - gf r) with
    gf r the largest taxed gain fraction x rate of the state; dust sub-case states (total > 1e-6 >= capacity) match to 1e-12."""
    rng = np.random.default_rng(SEED + int(rate * 1e9) % 1000)
    n = 1500
    for mask in (1, 2, 3):
        for alloc in (0.5, 0.999, 1.0):
            cfg = _helper_cfg(rate, mask, alloc)
            p = params_from_config(Config(**cfg))
            use1, r1 = cfg["inv1_use_realized_gains_tax_system"], cfg["inv1_realized_gains_tax_rate"]
            use2, r2 = cfg["inv2_use_realized_gains_tax_system"], cfg["inv2_realized_gains_tax_rate"]
            b1, c1, b2, c2, dust = _states(rng, n, rate)
            total = b1 + b2
            cap1, cap2 = _cap_ref(oracle, b1, c1, use1, r1), _cap_ref(oracle, b2, c2, use2, r2)
            cap = cap1 + cap2
            pick = rng.integers(0, 4, n)     # need at, below, above the capacity; zero
            need = np.select([pick == 0, pick == 1, pick == 2], [cap, cap * rng.uniform(0, 1, n), cap * rng.uniform(1, 3, n) + 2 * EPS], 0.0)
            got = E.eval_helper_host(N.MCR_HELPER_WITHDRAW_MONTH, p, np.column_stack((b1, c1, b2, c2, need)))
            exp = np.empty((n, 6))
            for i in range(n):
                target = max(0.0, min(need[i], cap[i]))
                prop1 = cap1[i] / cap[i] if cap[i] > EPS else alloc
                w1 = oracle.withdraw(b1[i], c1[i], target * prop1, use1, r1)
                w2 = oracle.withdraw(b2[i], c2[i], target * (1.0 - prop1), use2, r2)
                exp[i] = (w1[0], w1[1], w2[0], w2[1], w1[2] + w2[2], w1[3] + w2[3])
            gfr = np.zeros(n)
            for b, c, use, r in ((b1, c1, use1, r1), (b2, c2, use2, r2)):
                if use:
                    gf = np.where(b > 0, np.maximum(0.0, b - c) / np.where(b > 0, b, 1.0), 0.0)
                    gfr = np.maximum(gfr, gf * r)
            scale = np.maximum(np.maximum(total, c1 + c2), 1.0)
            bound = 16.0 * U * scale / np.maximum(EPS, 1.0 - gfr)
            sub = (total > EPS) & (cap <= EPS)           # the dust sub-case (reached on purpose: `dust` above)
            assert sub.sum() >= 10, (rate, mask, alloc, int(sub.sum()))
            for k, name in enumerate(("b1", "c1", "b2", "c2", "gross", "net")):
                err = np.abs(got[:, k] - exp[:, k])
                bad = np.nonzero(~sub & (err > bound))[0]
                assert bad.size == 0, ("withdraw month", name, rate, mask, alloc, bad[:4].tolist(), got[bad[:4], k].tolist(),
                                       exp[bad[:4], k].tolist(), bound[bad[:4]].tolist())
                bad = np.nonzero(sub & (err > 1e-12))[0]
                assert bad.size == 0, ("dust sub-case", name, rate, mask, alloc, bad[:4].tolist(), got[bad[:4], k].tolist(),
                                       exp[bad[:4], k].tolist())
            got = E.eval_helper_host(N.MCR_HELPER_REBALANCE_MONTH, p, np.column_stack((b1, c1, b2, c2)))
            exp = np.array([oracle.rebalance(p, b1[i], c1[i], b2[i], c2[i]) for i in range(n)])
            # the rebalance sells gf r x the SOLD asset's weight: 1 - a gf r >= 1 - gf r
            for k, name in enumerate(("b1", "c1", "b2", "c2")):
                err = np.abs(got[:, k] - exp[:, k])
                bad = np.nonzero(err > np.maximum(bound, 1e-12))[0]
                assert bad.size == 0, ("rebalance month", name, rate, mask, alloc, bad[:4].tolist(), got[bad[:4], k].tolist(),
                                       exp[bad[:4], k].tolist(), bound[bad[:4]].tolist())


def _path_cfg(family, rate, k):
    """k picks the taxed asset(s) and the allocation, so that every rate sees several of each."""
    mask = (1, 2, 3)[k % 3]
    d = dict(scenario="high_rate", contribution_growth_rate_annual=0.0, current_age=40.0,
             inv1_annual_tax_on_gains_rate=0.0, inv2_annual_tax_on_gains_rate=0.0,
             inv1_realized_gains_tax_rate=rate if mask & 1 else 0.2, inv1_use_realized_gains_tax_system=bool(mask & 1),
             inv2_realized_gains_tax_rate=rate if mask & 2 else 0.2, inv2_use_realized_gains_tax_system=bool(mask & 2),
             inflation_rate_mean=0.03, inflation_rate_volatility=0.01, equity_inflation_correlation=0.0,
             num_simulations_main=1, num_simulations_search=1, target_probability=50.0, starting_working_months_search=0,
             seed=None, num_processes=1, other_income_streams=[])
    if family == "gains":           # long accumulation at high means: the gain fraction nears 1 by retirement; ~30 % fail
        d.update(initial_balance=50_000.0, monthly_contribution=1_500.0, monthly_expenses=(2_300.0, 3_500.0, 900.0)[k % 3],
                 retirement_years=25, allocation_inv1_pct=(0.5, 0.999, 0.5)[k % 3],
                 inv1_returns_mean=0.14, inv1_returns_volatility=0.2,
                 inv2_premium_over_inflation_mean=0.09, inv2_premium_over_inflation_volatility=0.1)
        wm = 180
    elif family == "cents":         # fractions of a cent, 50 %+ means, both assets taxed: failing months reach capacity <= 1e-6 < total
        d.update(inv1_realized_gains_tax_rate=rate, inv1_use_realized_gains_tax_system=True,
                 inv2_realized_gains_tax_rate=rate, inv2_use_realized_gains_tax_system=True,
                 initial_balance=1e-3, monthly_contribution=0.0, monthly_expenses=3e-6,
                 retirement_years=20, allocation_inv1_pct=(0.5, 0.999, 0.7)[k % 3],
                 inv1_returns_mean=0.6, inv1_returns_volatility=0.5,
                 inv2_premium_over_inflation_mean=0.5, inv2_premium_over_inflation_volatility=0.4)
        wm = 36
    else:                           # rebalance-heavy: allocation 0.999 / 1.0, one asset taxed
        mask = 1 + k % 2
        d.update(inv1_realized_gains_tax_rate=rate if mask == 1 else 0.0, inv1_use_realized_gains_tax_system=mask == 1,
                 inv2_realized_gains_tax_rate=rate if mask == 2 else 0.0, inv2_use_realized_gains_tax_system=mask == 2,
                 initial_balance=200_000.0, monthly_contribution=500.0, monthly_expenses=700.0,
                 retirement_years=30, allocation_inv1_pct=(0.999, 1.0)[k % 2],
                 inv1_returns_mean=0.10, inv1_returns_volatility=0.25,
                 inv2_premium_over_inflation_mean=0.05, inv2_premium_over_inflation_volatility=0.15)
        wm = 60
    return d, wm


def _counts(p, seed, wm, n, env=None):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    try:
        r = E.run_batch_host(p, seed, 1, 0, n, wm, want_summary=False, want_trajectories=False)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return np.concatenate([r["counters"], r["ruin_year_bins"], r["wr_obs_counts"]]).astype(np.int64)


@pytest.mark.parametrize("rate", RATES)
def test_paths_at_high_rates_match_the_oracle_on_every_route(oracle, rate):
    """Per element 1e-9 (+1e-6) and identical flags, counters and bins — no knife-edge waiver: every money scale here is far
    below 2^33.  The plain launch, the search probes and the summary-only / count-only modes agree bit for bit (the time-sliced
    form needs a launch above the resident capacity: the next test).  Asserts that it reaches failing paths and, in the dust family, failing-year residuals in (1e-6, 1e-6 / (1 - r)]."""
    k = RATES.index(rate)
    stats = {"paths": 0, "failed": 0, "dust": 0, "worst": 0.0}
    for fi, family in enumerate(("gains", "cents", "rebalance")):
        cfgd, wm = _path_cfg(family, rate, k + fi)
        p = params_from_config(Config(**cfgd))
        seed = SEED + 7919 * k + fi
        n = N_PATHS
        g = E.run_batch_host(p, seed, 1, 0, n, wm)
        c = oracle.run_batch(p, seed, 1, 0, n, wm)
        ctx = (family, rate, wm, cfgd)
        scale = np.maximum(1.0, np.abs(c["trajectory"]).max(axis=0))     # the path's own money scale
        worst = max(float((np.abs(g[key] - c[key]) / scale).max()) for key in ("trajectory", "real_trajectory", "final_balance"))
        stats["worst"] = max(stats["worst"], worst)
        print(f"high-rate {family} r={rate!r}: failed {int((c['success'] == 0).sum())}/{n}, worst error / scale {worst:.3g}, "
              f"flag flips {int((g['success'] != c['success']).sum())}")
        for key in ("counters", "ruin_year_bins", "wr_obs_counts"):
            assert g[key].tolist() == c[key].tolist(), (ctx, key)
        assert np.array_equal(g["success"], c["success"]), (ctx, np.nonzero(g["success"] != c["success"])[0][:8].tolist())
        np.testing.assert_array_equal(g["years_to_ruin"], c["years_to_ruin"], err_msg=str(ctx))
        assert scale.max() < 2.0 ** 33, ctx
        for key in ("trajectory", "real_trajectory"):
            err = np.abs(g[key] - c[key])
            assert np.all(err <= ABS + REL * np.maximum(np.abs(c[key]), scale)), (ctx, key, float(err.max()))
        gw, cw = g["withdrawal_rate_trajectory"], c["withdrawal_rate_trajectory"]
        assert np.array_equal(np.isnan(gw), np.isnan(cw)), ctx
        np.testing.assert_allclose(gw, cw, rtol=1e-8, atol=1e-9, equal_nan=True, err_msg=str(ctx))
        for key in ("start_balance", "final_balance", "first_year_gross_withdrawal", "first_year_real_gross_withdrawal",
                    "inflation_at_retirement"):
            err = np.abs(g[key] - c[key])
            assert np.all(err <= ABS + REL * np.maximum(np.abs(c[key]), scale)), (ctx, key, float(err.max()))
        failed = c["success"] == 0
        stats["paths"] += n
        stats["failed"] += int(failed.sum())
        if family == "cents":
            top = EPS / (1.0 - rate) if rate < 1.0 else np.inf
            fb = c["final_balance"][failed]
            stats["dust"] += int(((fb > EPS) & (fb <= top)).sum())
            print(f"high-rate cents r={rate!r}: failing residuals in (1e-6, 1e-6 / (1 - r)]: {stats['dust']}")
        # the same inputs on the other routes: identical integers
        cnt = _counts(p, seed, wm, n)
        summ = E.run_batch_host(p, seed, 1, 0, n, wm, want_trajectories=False)
        for key in ("counters", "ruin_year_bins", "wr_obs_counts"):
            assert summ[key].tolist() == g[key].tolist(), (ctx, "summary-only", key)
        for key in E.SUMMARY_FIELDS + ("success",):
            assert np.array_equal(summ[key], g[key], equal_nan=True), (ctx, "summary-only", key)
        assert cnt.tolist() == np.concatenate([g["counters"], g["ruin_year_bins"], g["wr_obs_counts"]]).tolist(), (ctx, "count-only")
        months = [wm - 12, wm, wm + 1]
        probes = E.probe_months(p, seed, 1, 0, n, months).cpu().numpy()
        for m, row in zip(months, probes):
            one = E.run_batch_host(p, seed, 1, 0, n, m, want_summary=False, want_trajectories=False)
            assert row.tolist() == one["counters"].tolist(), (ctx, "probe", m)
        assert probes[1].tolist() == g["counters"].tolist(), (ctx, "probe")
    print(f"high-rate paths r={rate!r}: {stats}")
    assert stats["failed"] >= 0.1 * stats["paths"], stats
    if rate >= 0.999:   # (at 0.99 the band (1e-6, 1e-4] is narrower than one month's withdrawal: the family does not fail)
        assert stats["dust"] >= 30, stats


@pytest.mark.parametrize("rate", [0.999, 1 - 2e-6, 1 - 1e-6])
def test_time_sliced_launch_counts_equal_the_plain_launch_at_high_rates(rate):
    """The time-sliced form (PHASE 3, csrc/mcr_hip.hip plan_segments) carries the slow month and its dust branch across
    segment hand-overs: 400 000 count-only paths (above the resident capacity of 256 CUs x 6 workgroups, so the launcher
    cuts blocks into segments when told to) give the same integers as the plain launch — with the hand-over through memory
    and with every successor recomputing its block.  The cents family must reach the dust band in this very launch."""
    n = 400_000
    for fi, family in enumerate(("gains", "cents")):
        cfgd, wm = _path_cfg(family, rate, RATES.index(rate) + fi)   # (the configurations of the oracle test above)
        p = params_from_config(Config(**cfgd))
        seed = SEED + 104729 + fi
        plain = _counts(p, seed, wm, n, {"MCR_K1_SEGMENTS": "0"})
        assert int(plain[1]) == n and 0.1 * n < n - int(plain[0]), (family, rate, plain[:2].tolist())
        for env in ({"MCR_K1_SEGMENTS_ALWAYS": "1"}, {"MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENT_POLLS": "0"}):
            got = _counts(p, seed, wm, n, env)
            assert np.array_equal(got, plain), (family, rate, env, np.nonzero(got != plain)[0][:8].tolist())
        if family == "cents":
            res = E.run_batch_host(p, seed, 1, 0, n, wm, want_trajectories=False)
            fb = res["final_balance"][res["success"] == 0]
            assert int(((fb > EPS) & (fb <= EPS / (1.0 - rate))).sum()) >= 300, rate
