"""The screening kernel's path in plain NumPy — a helper of the screened-route tests, not a test.

`model` restates what csrc/mcr_screen.h and the comment above screen_kernel (csrc/mcr_hip.hip) SAY the kernel computes, one
path per array element and one month per loop turn, from the plan's parameters and the oracle's own shocks
(`oracle.draw_shocks`, which has mixed rho in).  It is written from that description and not from the kernel's instruction
sequence: plain products, quotients and sums, no fused operations, exp rather than a pre-scaled exp2.

    growth      g1 = exp(mu1 / 12 + sigma1 / sqrt(12) z_equity), likewise inflation and the premium; asset 2 grows by
                inflation x premium
    accumulate  the contribution grows once every twelve accumulation months (the kernel's `moy` counter), then
                balance x growth, + the contribution split by the allocation, to balance and cost basis alike
    decumulate  price = the price level BEFORE the month's growth; need = max(0, expenses x price - netted amount x price of
                each indexed income record whose window holds the month); growth; capacity = what both assets fetch
                after the realized-gains tax; the two tests; sell the fraction min(need, capacity) / capacity of both assets
    rebalance   sell the asset above its allocation down to it, net of the tax on the sold fraction's gain, and buy the
                other with the proceeds (every month); `peak` is the running maximum of b1 + b2 before that trade
    SAFE        min(b1, b2) > 1 at the start and after every month's rebalance; in every retirement month
                capacity >= 24 need and capacity >= peak / 64; and peak < 1e30 at the end

The rebalance that closes a tax year and the dust fix-ups of the fp64 month are left out, as the kernel leaves them out.

`slack` is the path's decisive margin: the minimum over all those tests of (left side) / (right side).  A path is SAFE when
every test holds, so `slack >= 1` for a SAFE path and `slack <= 1` for a DOUBTFUL one, and two runs of the loop in different
precisions can disagree on a path's class only where `slack` is within their deviation of 1.

`dtype=np.float32` runs the same loop in single precision: the parameters are derived in double and rounded once (as
screen_params does), and every array is cast back to `dtype` each month, because NumPy promotes silently where a Python
scalar or a double meets a single (`np.where`, products with constants).
"""

from __future__ import annotations

import math
from typing import Dict

import numpy as np

from monte_carlo_retirement_amd import engine as E
from oracle import oracle as O

NEED_MARGIN = 24.0        # kScreenNeedMargin
PEAK_DIV = 64.0           # kScreenPeakDiv
MIN_BALANCE = 1.0         # kScreenMinBalance
MAX_TOTAL = 1e30          # kScreenMaxTotal
MONTHS_PER_YEAR = 12

_SHOCKS = {}


def shocks(params, wm: int, seed: int, stream: int, begin: int, n: int) -> np.ndarray:
    """[n, total_months, 3] float64 (equity, inflation with rho mixed in, premium): the oracle's shocks of the path range."""
    total = int(wm) + int(params.retirement_years) * MONTHS_PER_YEAR
    key = (int(seed), int(stream), int(begin), int(n), total, float(params.equity_inflation_rho))
    if key not in _SHOCKS:
        _SHOCKS[key] = np.stack([O.draw_shocks(int(seed), int(stream), int(begin) + i, total, float(params.equity_inflation_rho))
                                 for i in range(int(n))])
    return _SHOCKS[key]


def income_windows(params, cfgd: dict, wm: int):
    """[(netted amount, first row, one past the last row)] of the records `engine.kept_streams` keeps; rows count from month 0
    of the path, and a record without a duration never ends."""
    out = []
    for index, slot in E.kept_streams(params, wm):
        rec = cfgd["other_income_streams"][index]
        assert slot == -1 and rec["inflation_indexed"], "the screening month has indexed income records only"
        first = int(wm) + O.stream_start_month_index(float(cfgd["current_age"]), int(wm), float(rec["start_at_age"]))
        years = rec["duration_years"]
        end = math.inf if years is None else first + int(years) * MONTHS_PER_YEAR
        out.append((float(rec["monthly_amount_today"]) * (1.0 - float(rec["tax_rate"])), first, end))
    assert len(out) <= 2, "the screening month carries at most two income records"
    return out


def _effective_rate(use_realized, rate: float) -> float:
    return float(rate) if use_realized and rate > 0.0 else 0.0


def model(params, cfgd: dict, wm: int, seed: int, stream: int, begin: int, n: int, dtype=np.float64) -> Dict[str, np.ndarray]:
    """Per path of [begin, begin + n): `safe` (bool), `slack`, `min_ratio` (lowest capacity / need over the retirement months
    with a need; inf without one) and `final_total` (b1 + b2 after the last month), computed in `dtype`."""
    dt = np.dtype(dtype).type
    cast = lambda x: np.asarray(x, dtype=dt)        # noqa: E731
    wm, n = int(wm), int(n)
    total_months = wm + int(params.retirement_years) * MONTHS_PER_YEAR
    z = shocks(params, wm, seed, stream, begin, n)
    sqrt12 = math.sqrt(MONTHS_PER_YEAR)
    a1, s1 = dt(params.inv1_mu_log / MONTHS_PER_YEAR), dt(params.inv1_sigma_log / sqrt12)
    ai, si = dt(params.inf_mu_log / MONTHS_PER_YEAR), dt(params.inf_sigma_log / sqrt12)
    ap, sp = dt(params.prem_mu_log / MONTHS_PER_YEAR), dt(params.prem_sigma_log / sqrt12)
    alloc1 = dt(params.allocation_inv1_pct)
    rate1 = _effective_rate(params.inv1_use_realized_gains_tax_system, params.inv1_realized_gains_tax_rate)
    rate2 = _effective_rate(params.inv2_use_realized_gains_tax_system, params.inv2_realized_gains_tax_rate)
    # allocation x rate of the asset sold: the tax on the sold gain shrinks the total that the allocation is a share of
    w1, w2 = dt(params.allocation_inv1_pct * rate1), dt((1.0 - params.allocation_inv1_pct) * rate2)
    rate1, rate2 = dt(rate1), dt(rate2)
    expenses = dt(params.monthly_expenses)
    windows = [(dt(a), first, end) for a, first, end in income_windows(params, cfgd, wm)]
    grows = params.contribution_growth_rate_annual > 0
    growth = dt(1.0 + params.contribution_growth_rate_annual)
    contrib = dt(params.monthly_contribution)
    zero, one = dt(0.0), dt(1.0)
    margin, peak_div, min_balance = dt(NEED_MARGIN), dt(PEAK_DIV), dt(MIN_BALANCE)

    first = params.initial_balance * params.allocation_inv1_pct
    b1 = np.full(n, dt(first), dtype=dt)
    b2 = np.full(n, dt(params.initial_balance - first), dtype=dt)
    c1, c2 = b1.copy(), b2.copy()
    price_level = np.ones(n, dtype=dt)
    peak = cast(b1 + b2)
    low = np.minimum(b1, b2)
    safe = low > min_balance
    slack = cast(low / min_balance)
    min_ratio = np.full(n, np.inf, dtype=dt)
    moy = 0

    with np.errstate(all="ignore"):
        for m in range(total_months):
            ze, zi, zp = cast(z[:, m, 0]), cast(z[:, m, 1]), cast(z[:, m, 2])
            g1 = cast(np.exp(cast(a1 + cast(s1 * ze))))
            ginf = cast(np.exp(cast(ai + cast(si * zi))))
            g2 = cast(ginf * cast(np.exp(cast(ap + cast(sp * zp)))))
            if m < wm:
                if moy == MONTHS_PER_YEAR:
                    moy = 0
                    if grows:
                        contrib = dt(contrib * growth)
                moy += 1
                k1 = dt(contrib * alloc1)
                k2 = dt(contrib - k1)
                b1, b2, price_level = cast(b1 * g1), cast(b2 * g2), cast(price_level * ginf)
                b1, c1, b2, c2 = cast(b1 + k1), cast(c1 + k1), cast(b2 + k2), cast(c2 + k2)
            else:
                price = price_level
                net = cast(expenses * price)
                for amount, start, end in windows:
                    if start <= m < end:
                        net = cast(net - cast(amount * price))
                need = cast(np.maximum(zero, net))
                b1, b2, price_level = cast(b1 * g1), cast(b2 * g2), cast(price_level * ginf)
                v1 = cast(b1 - cast(np.maximum(zero, cast(b1 - c1)) * rate1))
                v2 = cast(b2 - cast(np.maximum(zero, cast(b2 - c2)) * rate2))
                cap = cast(v1 + v2)
                safe &= (cap >= cast(margin * need)) & (cap >= cast(peak / peak_div))
                has_need = need > zero
                ratio = cast(np.where(has_need, cast(cap / need), np.inf))
                min_ratio = cast(np.fmin(min_ratio, ratio))
                slack = cast(np.fmin(slack, np.fmin(cast(ratio / margin), cast(cap / cast(peak / peak_div)))))
                sold = cast(cast(np.minimum(need, cap)) / cap)
                keep = cast(one - sold)
                b1, c1, b2, c2 = cast(b1 * keep), cast(c1 * keep), cast(b2 * keep), cast(c2 * keep)
            # the month's rebalance: sell what stands above its allocation, net of the tax on the sold gain
            total = cast(b1 + b2)
            drift1 = cast(b1 - cast(total * alloc1))
            sell1 = drift1 > zero
            bs, cs = cast(np.where(sell1, b1, b2)), cast(np.where(sell1, c1, c2))
            rate_s, w_s = cast(np.where(sell1, rate1, rate2)), cast(np.where(sell1, w1, w2))
            gain = cast(np.maximum(zero, cast(bs - cs)))
            fraction = cast(np.minimum(one, cast(np.abs(drift1) / cast(bs - cast(w_s * gain)))))
            bought = cast(fraction * cast(bs - cast(gain * rate_s)))
            left = cast(one - fraction)
            nbs, ncs = cast(bs * left), cast(cs * left)
            b1, c1, b2, c2 = (cast(np.where(sell1, nbs, cast(b1 + bought))), cast(np.where(sell1, ncs, cast(c1 + bought))),
                              cast(np.where(sell1, cast(b2 + bought), nbs)), cast(np.where(sell1, cast(c2 + bought), ncs)))
            peak = cast(np.maximum(peak, total))
            low = np.minimum(b1, b2)
            safe &= low > min_balance
            slack = cast(np.fmin(slack, cast(low / min_balance)))
        safe &= peak < dt(MAX_TOTAL)
        slack = cast(np.fmin(slack, cast(dt(MAX_TOTAL) / peak)))
        final_total = cast(b1 + b2)
    # (a ruined path divides 0 by 0 from its ruin on: its comparisons are false from then on, and np.fmin keeps the slack and
    # the ratio it had, as the kernel's minimum does)
    safe &= np.isfinite(final_total)
    return {"safe": safe, "slack": slack, "min_ratio": min_ratio, "final_total": final_total}
